// lstm_dev.h -- device-side data model for the LSTM recurrent path (reference: NeuralAudio/LSTM.h,
// NeuralAudio/LSTMDynamic.h -- same arithmetic).
//
// Mapping: the recurrence is strictly sample-serial inside a stream, so parallelism comes from
// streams only: one lane = one stream, 64 streams per wave64.  Weights are wave-uniform (scalar
// loads / SGPR broadcast), h and c live in LDS as [element][lane] (conflict-free columns) and are
// pulled into VGPRs for each gate mat-vec.
//
// HBM state per model group: float state[(layer*2H + k) * capacity + slot], k < H: hidden, k >= H: cell
// (structure-of-arrays over streams so a wave's 64 lanes load/store 256 contiguous bytes).
#pragma once

#include <algorithm>
#include <cstdlib>

#include "tuning.h"

namespace na
{
	constexpr int LSTM_MAX_LAYERS = 8;
	constexpr int LSTM_MAX_FRAMES = 128;
	constexpr int LSTM_MAX_TAIL = 8;        // dense layers of a generic keras stack (after lowering: activation / batchnorm / prelu layers become dense ones)
	constexpr int LSTM_MAX_TAIL_WIDTH = 256; // units per dense layer (two [width][64] scratch arrays in LDS: the shape predicates below check the fit)
	constexpr int LSTM_MAX_TAIL_HISTORY = 1024; // conv1d layers of a keras stack: (taps - 1) x dilation samples of input history at most

	enum { LSTM_CELL_LSTM = 0, LSTM_CELL_GRU = 1 };
	enum { LSTM_MATH_FAST = 0, LSTM_MATH_STD = 1 };

	// Shapes with a kernel (host-side predicates, no HIP types: the loader rejects everything else at load time).
	//   LSTM: any hidden size / layer count whose lane = stream working set fits the 160 KB LDS (LstmGenericKernel); the usual sizes
	//   have shaped kernels.  GRU: likewise (GruGenericKernel; GruWaveKernel / DPP instances for 1-2 layers of 8, 12, 16, 20).
	// tailWidth: widest dense layer of a generic keras stack (0: the classic 1-unit head); such a model may have no recurrent layer
	//   Round 3: the runtime-shaped wave kernel streams weights that do not fit the LDS from L2 (RecurrentWaveRtKernel, weights
	//   transposed for coalesced reads), so every shape up to RECURRENT_WAVE_MAX_HIDDEN units has a real-time kernel whatever the
	//   weight size (LSTMDynamic.h:95-108,166-179 runs any size on the CPU).
	//   Round 4: from 65 gate rows on (LSTM / GRU of more than 16 / 21 units on this kernel) a stream is a WORKGROUP of 2 .. 16 waves that share the
	//   gate rows (RecurrentWaveWaves; a barrier where the one-wave version has a wave fence), so the limit is 1024 units; beyond 128
	//   units the 1-unit head is evaluated inside the sample loop (no [samples][H] buffer) and a dense tail needs that buffer to fit.
	constexpr int RECURRENT_WAVE_MAX_HIDDEN = 1024;
	constexpr int RECURRENT_HEAD_IN_LOOP_FROM = 129; // hidden sizes from here on: classic head inside the sample loop
	constexpr long RECURRENT_LDS_BYTES = 160L * 1024;
#ifdef __HIPCC__
#define NA_HOST_DEVICE __host__ __device__
#else
#define NA_HOST_DEVICE
#endif
	// the classic 1-unit head inside the sample loop (no [samples][H] buffer): wide layers without a dense / conv1d tail
	NA_HOST_DEVICE inline bool RecurrentHeadInLoop(int hidden, bool hasTail) { return hidden >= RECURRENT_HEAD_IN_LOOP_FROM && !hasTail; }
	// gate rows per lane of a stream's threads (the kernel's GateRowsL2Dispatch case; the LDS path strides its rows the same way)
	NA_HOST_DEVICE inline int RecurrentRowsPerLane(int gateRows, int threads) { return (gateRows + threads - 1) / threads; }
	// waves per stream of the runtime-shaped kernel: one gate row per lane up to 16 waves (the kernel is bound by the latency of its
	// weight loads from L2, and more waves keep more of them in flight: LSTM 1x256 x 64 streams 2.32 / 1.63 / 1.34 ms per 128-sample
	// block at four / two / one row per lane, LSTM 1x128 1.22 / 0.90 / 0.68; round 3, one wave: 2.0)
	inline int RecurrentWaveWaves(int gateRows, int rpl)
	{
		int waves = 1;
		while (waves < 16 && gateRows > 64 * rpl * waves) waves *= 2;
		return waves;
	}
	// tailHistory > 0: the tail has conv1d layers -- it is evaluated layer by layer over the whole block (recurrent_tail.h ConvTail) and its two
	// scratch arrays are [tailWidth][tailHistory + 128] (tailWidth then covers the widest INPUT of a tail layer as well)
	NA_HOST_DEVICE inline long RecurrentTailScratchFloats(int tailWidth, int tailHistory) { return tailHistory > 0 ? 2L * tailWidth * (tailHistory + LSTM_MAX_FRAMES) : 2L * tailWidth * 64; }
	// LDS floats of RecurrentWaveRtKernel (its layout: lstm_kernels.hip), with or without the gate weights of all layers
	// (tailWidth / tailHistory: 0 without a tail)
	inline long RecurrentWaveLdsFloats(int cell, int hidden, int numLayers, int tailWidth, int tailHistory, bool hasTail, bool weightsInLds)
	{
		const long H = hidden, L = numLayers;
		const long rowsPerLayer = (cell == LSTM_CELL_GRU ? 3 : 4) * H, biases = (cell == LSTM_CELL_GRU ? 6 : 4) * H;
		const bool hseq = !RecurrentHeadInLoop(hidden, hasTail);
		long f = LSTM_MAX_FRAMES + 2 * L * H + 6 * H + (hseq ? 2 * (L > 0 ? H : 1) * 64 : 0) + RecurrentTailScratchFloats(tailWidth, tailHistory);
		if (weightsInLds)
			for (int l = 0; l < numLayers; l++) f += rowsPerLayer * (long)(((l == 0 ? 1 : hidden) + hidden) | 1) + biases;
		return f;
	}
	inline bool RecurrentWaveShape(int hidden, int numLayers, int tailWidth, int tailHistory = 0)
	{
		if (!(hidden >= 1 && hidden <= RECURRENT_WAVE_MAX_HIDDEN && numLayers >= (tailWidth > 0 ? 0 : 1) && numLayers <= LSTM_MAX_LAYERS &&
			tailWidth <= std::max(LSTM_MAX_TAIL_WIDTH, tailHistory > 0 ? hidden : 0) && tailHistory <= LSTM_MAX_TAIL_HISTORY)) return false;
		// LDS without the weights (they stream from L2 when they do not fit): xin | h, c | gates | [samples][H] of the last layer (small models
		// and dense tails) | tail scratch
		const bool hseq = !RecurrentHeadInLoop(hidden, tailWidth > 0);
		const long floats = LSTM_MAX_FRAMES + 2L * numLayers * hidden + 6L * hidden + (hseq ? 2L * (numLayers > 0 ? hidden : 1) * 64 : 0) +
			RecurrentTailScratchFloats(tailWidth, tailHistory) + 64;
		return floats * 4 <= RECURRENT_LDS_BYTES;
	}
	// shapes of the LDS-free kernels (recurrent_dpp_kernels.hip RecurrentDppSupported): hidden sizes below a layout (8 or 16 units per gate
	// block) are padded into it: 12 (the reference's static 1x12 / 2x12) runs as 16 ... and one-layer LSTMs (the reference's static 1x24) /
	// keras GRUs of 17 .. 32 units on the 32-unit layout (noDpp32: the tuning knob NA_REC_NO_DPP32 takes that layout away)
	inline bool RecurrentDppShape(int cell, int hidden, int numLayers, int tailLayers, bool noDpp32)
	{
		if (tailLayers != 0) return false; // generic keras stacks run on the runtime-shaped kernels
		if (cell != LSTM_CELL_LSTM && cell != LSTM_CELL_GRU) return false;
		if (numLayers == 1 && hidden > 16 && hidden <= 32) return !noDpp32;
		return hidden >= 1 && hidden <= 16 && (numLayers == 1 || numLayers == 2);
	}
	// the shaped one-wave instances (LstmWaveKernel<H, L> / GruWaveKernel<H, L>) and the shaped lane = stream ones (LstmBlockKernel<H>): the
	// decision below and the instantiation switches of the kernel files both read these
	inline bool LstmWaveShape(int hidden, int numLayers)
	{
		return (hidden == 8 || hidden == 12 || hidden == 16 || hidden == 20 || hidden == 24 || hidden == 32) && (numLayers == 1 || numLayers == 2);
	}
	inline bool GruWaveShape(int hidden, int numLayers) { return (hidden == 8 || hidden == 12 || hidden == 16 || hidden == 20) && (numLayers == 1 || numLayers == 2); }
	inline bool LstmBlockShape(int hidden) { return hidden == 4 || hidden == 40 || LstmWaveShape(hidden, 1); }
	// dynamic LDS of the lane = stream kernels for a block of n samples (state of 64 streams in LDS; tailWidth: 0 without a dense tail).
	// RecurrentKernelFor chooses these kernels only where the longest block (n = LSTM_MAX_FRAMES) fits, so the launchers' own checks of
	// the block at hand (the kernels' bound, kept beside them) cannot fail behind a choice
	inline long LstmBlockLdsBytes(int hidden, int numLayers, int n) { return (64L * (n + 1) + (long)numLayers * 2 * hidden * 64) * 4; }
	inline long LstmGenericLdsBytes(int hidden, int numLayers, int n, int tailWidth) { return LstmBlockLdsBytes(hidden, numLayers, n) + ((long)hidden * 64 + 2L * tailWidth * 64) * 4; }
	inline long GruGenericLdsBytes(int hidden, int numLayers, int n, int tailWidth) { return (64L * (n + 1) + (long)numLayers * hidden * 64 + 6L * hidden * 64 + 2L * tailWidth * 64) * 4; }
	// the lane = stream kernels' bound (LstmGenericKernel / GruGenericKernel at the longest block)
	inline bool LstmLaneKernelShape(int hidden, int numLayers, int tailWidth = 0)
	{
		if (hidden < 1 || numLayers < (tailWidth > 0 ? 0 : 1) || numLayers > LSTM_MAX_LAYERS || tailWidth > LSTM_MAX_TAIL_WIDTH) return false;
		return LstmGenericLdsBytes(hidden, numLayers, LSTM_MAX_FRAMES, tailWidth) <= RECURRENT_LDS_BYTES;
	}
	inline bool GruLaneKernelShape(int hidden, int numLayers, int tailWidth = 0)
	{
		if (hidden < 1 || numLayers < 1 || numLayers > LSTM_MAX_LAYERS || tailWidth > LSTM_MAX_TAIL_WIDTH) return false;
		return GruGenericLdsBytes(hidden, numLayers, LSTM_MAX_FRAMES, tailWidth) <= RECURRENT_LDS_BYTES;
	}
	// what the loader admits (knob-independent; a tail with conv1d layers -- tailHistory > 0 -- only runs on the runtime-shaped wave kernel)
	inline bool LstmShapeSupported(int hidden, int numLayers, int tailWidth = 0, int tailHistory = 0)
	{
		return (tailHistory == 0 && LstmLaneKernelShape(hidden, numLayers, tailWidth)) || RecurrentWaveShape(hidden, numLayers, tailWidth, tailHistory);
	}
	inline bool GruShapeSupported(int hidden, int numLayers, int tailWidth = 0, int tailHistory = 0)
	{
		return (tailHistory == 0 && GruLaneKernelShape(hidden, numLayers, tailWidth)) || (numLayers >= 1 && RecurrentWaveShape(hidden, numLayers, tailWidth, tailHistory));
	}

	// How the runtime-shaped kernel (RecurrentWaveRtKernel) runs a model: the kernel shares RecurrentHeadInLoop / RecurrentRowsPerLane /
	// RecurrentWaveLdsFloats' layout.
	struct RecurrentPlan
	{
		int runs;        // 1: RecurrentKernelFor chose this kernel (0: another kernel runs the model; the rest is then what this kernel WOULD do)
		int waves;       // waves per stream: 1 = RecurrentWaveRtKernel<64> (wave fences), 2 .. 16 = <1024> (barriers)
		int rowsPerLane; // gate rows per lane, 1 .. 8
		int l2w;         // 1: the gate weights are streamed transposed from L2, 0: they sit in LDS
		int headInLoop;  // 1: the 1-unit head is evaluated inside the sample loop by the first wave
		long ldsBytes;   // dynamic LDS of the launch
	};

	// THE decision of which kernel runs a recurrent model, in one place: the group (gpu_groups.h LstmGroup) asks once and keeps the answer,
	// the launcher (recurrent_launch.cpp) switches on it, NA_BatchStreamKernelName reports it, the test hooks (NA_DebugRecurrentKernel,
	// NA_DebugRecurrentPlan) ask it about any shape and knob set.  No HIP types, no environment: a pure function that works without a device.
	enum class RecurrentKernel { None, Dpp, LstmWave, GruWave, WaveRt, LstmBlock, LstmGeneric, GruGeneric };
	inline const char* RecurrentKernelName(RecurrentKernel k)
	{
		static const char* const names[] = { "", "RecurrentDppKernel", "LstmWaveKernel", "GruWaveKernel", "RecurrentWaveRtKernel", "LstmBlockKernel", "LstmGenericKernel", "GruGenericKernel" };
		return names[(int)k];
	}
	// the tuning knobs that bear on the choice (tuning.h: NA_LSTM_NO_DPP, NA_GRU_NO_DPP, NA_LSTM_LANE_KERNEL, NA_LSTM_NO_WAVE_RT, NA_REC_NO_DPP32, NA_REC_RPL, NA_REC_L2W)
	struct RecurrentKnobs
	{
		bool lstmNoDpp = false, gruNoDpp = false, lstmLaneKernel = false, lstmNoWaveRt = false, recNoDpp32 = false;
		int recRpl = 1;
		bool recL2w = false;
		static RecurrentKnobs FromTuning()
		{
			const Tuning& t = Tuning::Get();
			return { t.lstmNoDpp, t.gruNoDpp, t.lstmLaneKernel, t.lstmNoWaveRt, t.recNoDpp32, t.recRpl, t.recL2w };
		}
	};
	struct RecurrentChoice
	{
		RecurrentKernel kernel; // None: no kernel takes the shape under these knobs (the launch is an error)
		RecurrentPlan plan;     // the runtime-shaped kernel's plan (plan.runs == (kernel == WaveRt))
	};
	// haveWT: the transposed weight image exists (LstmModelDev::wT)
	inline RecurrentChoice RecurrentKernelFor(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, bool haveWT, const RecurrentKnobs& k)
	{
		const bool gru = cell == LSTM_CELL_GRU, hasTail = tailLayers > 0, convTail = hasTail && tailHistory > 0;
		const int tw = hasTail ? tailWidth : 0, th = hasTail ? tailHistory : 0;
		const int gateRows = (gru ? 3 : 4) * hidden;
		RecurrentPlan p = {};
		p.waves = RecurrentWaveWaves(gateRows, k.recRpl > 0 ? k.recRpl : 1);
		p.rowsPerLane = RecurrentRowsPerLane(gateRows, 64 * p.waves);
		p.headInLoop = RecurrentHeadInLoop(hidden, hasTail) ? 1 : 0;
		p.ldsBytes = RecurrentWaveLdsFloats(cell, hidden, numLayers, tw, th, hasTail, true) * 4;
		// weights larger than the LDS (LSTM 2x64: 197 KB): streamed from L2, transposed for coalesced reads (NA_REC_L2W=1 forces the mode)
		p.l2w = (p.ldsBytes > RECURRENT_LDS_BYTES || (k.recL2w && numLayers > 0)) ? 1 : 0;
		if (p.l2w) p.ldsBytes = RecurrentWaveLdsFloats(cell, hidden, numLayers, tw, th, hasTail, false) * 4;
		// the runtime-shaped kernel takes the model: tuning knobs send models to the lane = stream kernels -- except tails with conv1d layers,
		// which only this kernel evaluates
		const bool rtFits = !((k.lstmNoWaveRt || (!gru && k.lstmLaneKernel)) && !convTail) && hidden >= 1 && hidden <= RECURRENT_WAVE_MAX_HIDDEN && numLayers >= 0 &&
			!(numLayers == 0 && !hasTail) && (!p.l2w || haveWT) && p.ldsBytes <= RECURRENT_LDS_BYTES;
		// the LDS-free kernels and the shaped one-wave instances come first (models without a tail); the lane = stream kernels last
		const bool dpp = !(gru ? k.gruNoDpp : k.lstmNoDpp) && RecurrentDppShape(cell, hidden, numLayers, tailLayers, k.recNoDpp32);
		RecurrentKernel kernel = RecurrentKernel::None;
		if (gru)
		{
			if (!GruShapeSupported(hidden, numLayers, tw, th)) kernel = RecurrentKernel::None;
			else if (dpp) kernel = RecurrentKernel::Dpp;
			else if (!hasTail && GruWaveShape(hidden, numLayers)) kernel = RecurrentKernel::GruWave;
			else if (rtFits) kernel = RecurrentKernel::WaveRt;
			else if (!convTail && GruGenericLdsBytes(hidden, numLayers, LSTM_MAX_FRAMES, tw) <= RECURRENT_LDS_BYTES) kernel = RecurrentKernel::GruGeneric;
		}
		else
		{
			const bool lane = k.lstmLaneKernel && !convTail; // NA_LSTM_LANE_KERNEL: the lane = stream kernels for everything they evaluate
			if (!lane && dpp) kernel = RecurrentKernel::Dpp;
			else if (!lane && !hasTail && LstmWaveShape(hidden, numLayers)) kernel = RecurrentKernel::LstmWave;
			else if (rtFits) kernel = RecurrentKernel::WaveRt;
			else if (convTail) kernel = RecurrentKernel::None;
			else if (!hasTail && LstmBlockShape(hidden)) kernel = LstmBlockLdsBytes(hidden, numLayers, LSTM_MAX_FRAMES) <= RECURRENT_LDS_BYTES ? RecurrentKernel::LstmBlock : RecurrentKernel::None;
			else if (LstmGenericLdsBytes(hidden, numLayers, LSTM_MAX_FRAMES, tw) <= RECURRENT_LDS_BYTES) kernel = RecurrentKernel::LstmGeneric;
		}
		p.runs = kernel == RecurrentKernel::WaveRt ? 1 : 0;
		return { kernel, p };
	}
	// The runtime-shaped kernel's plan alone, under the process's tuning knobs.  rpl > 0 / forceL2w >= 0: these instead of NA_REC_RPL /
	// NA_REC_L2W (tests ask for the default plan of a shape whatever the environment says)
	inline RecurrentPlan RecurrentWavePlan(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, bool haveWT = true,
		int rpl = 0, int forceL2w = -1)
	{
		RecurrentKnobs k = RecurrentKnobs::FromTuning();
		if (rpl > 0) k.recRpl = rpl;
		if (forceL2w >= 0) k.recL2w = forceL2w != 0;
		return RecurrentKernelFor(cell, hidden, numLayers, tailLayers, tailWidth, tailHistory, haveWT, k).plan;
	}

	struct LstmModelDev
	{
		// packed per layer l: W row-major [4H][I_l + H] (gate row blocks i,f,g,o -- LSTM.h:33-36), then bias[4H];
		// after the last layer: head weights [H], head bias [1]
		// GRU (cell == LSTM_CELL_GRU): per layer W row-major [3H][I_l + H] (gate row blocks z,r,c), then b_in[3H], b_rec[3H]
		const float* w;
		int cell;
		int numLayers;
		int hidden;
		int layerOff[LSTM_MAX_LAYERS]; // float offset of layer l's W
		int headOff;
		int math;      // LSTM only: 0 = FastMath (Activation.h:83-96), 1 = StdMath (Activation.h:20-45) -- the reference's LSTM_MATH build option
		// generic keras stack: tailLayers > 0 replaces the head by a chain of dense layers, layer t = W row-major [out][in] at
		// tailOff[t], then bias[out]; activation codes = DenseActivation (model_desc.h).  Only the runtime-shaped kernels evaluate it.
		int tailLayers;
		int tailOff[LSTM_MAX_TAIL], tailIn[LSTM_MAX_TAIL], tailOut[LSTM_MAX_TAIL], tailAct[LSTM_MAX_TAIL];
		int tailWidth; // widest layer (with conv1d layers: widest input or output of a tail layer)
		// conv1d layers of the tail (recurrent_tail.h ConvTail): taps / dilation per layer (1 / 1: a dense layer; weights [out][taps][in]), the
		// state row where the layer's input history starts (history x in rows, oldest sample first, behind the recurrent state's rows) and
		// the longest history (0: the tail has no conv1d layer)
		int tailK[LSTM_MAX_TAIL], tailDil[LSTM_MAX_TAIL], tailHistRow[LSTM_MAX_TAIL];
		int tailHistMax;
		// the same gate matrices transposed for the wave kernel's L2-streamed mode (weights larger than the LDS): per layer
		// [Qi + Qh][rowsPad][4] floats -- quad q of row r = weights of inputs 4q .. 4q + 3 (input part padded to Qi = ceil(I / 4) quads, hidden
		// part to Qh = ceil(H / 4)), rows padded to a multiple of 64: the 64 lanes of a wave read 64 consecutive rows of one quad = 1 KB
		const float* wT;
		int layerOffT[LSTM_MAX_LAYERS]; // float offsets into wT
		int rowsPad; // (a multiple of 64 x waves)
		int waves;   // waves per stream of the runtime-shaped kernel (RecurrentPlan::waves)
	};
}
