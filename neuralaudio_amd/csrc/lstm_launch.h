// lstm_launch.h -- host-callable launchers for the kernels in lstm_kernels.hip
#pragma once

#include <hip/hip_runtime_api.h>

#include "lstm_dev.h"

namespace na
{

	// One block of n samples for `numStreams` streams of one model: what every recurrent launcher below takes
	struct RecurrentBlock
	{
		const LstmModelDev& m;
		float* state;
		int capacity;
		const int *slots, *rows;
		int numStreams;
		const float* in;
		float* out;
		long inStride, outStride;
		int n;
		hipStream_t stream;
	};
	// ... on the kernel that RecurrentKernelFor chose for the model (lstm_dev.h; recurrent_launch.cpp: a switch, the guards on n and the
	// stream count).  The launchers behind it, one per kernel and without policy: lstm_kernels.hip, gru_kernels.hip
	hipError_t LaunchRecurrentBlock(const RecurrentChoice& choice, const RecurrentBlock& b);
	hipError_t LaunchLstmWave(const RecurrentBlock& b);    // LstmWaveKernel<H, L>: the shapes of LstmWaveShape
	hipError_t LaunchLstmBlockH(const RecurrentBlock& b);  // LstmBlockKernel<H>: the sizes of LstmBlockShape
	hipError_t LaunchLstmGeneric(const RecurrentBlock& b); // LstmGenericKernel
	hipError_t LaunchGruWave(const RecurrentBlock& b);     // GruWaveKernel<H, L>: the shapes of GruWaveShape
	hipError_t LaunchGruGeneric(const RecurrentBlock& b);  // GruGenericKernel
	// RecurrentWaveRtKernel<64 | 1024>: LSTM or GRU cells, any layer count, classic head or dense / conv1d chain, as `plan` lays it out
	hipError_t LaunchRecurrentWaveRt(const RecurrentPlan& plan, const RecurrentBlock& b);

	// LDS-free kernels for hidden size 8 / 16, 1-2 layers, LSTM or GRU (recurrent_dpp_kernels.hip): one launch over several model groups
	constexpr int RECURRENT_MAX_GROUPS = 8;
	struct RecurrentGroup
	{
		LstmModelDev model;
		float* state;
		int capacity;
		const int* slots; // nullptr: the active streams are contiguous -- stream i uses state slot slot0 + i and matrix row row0 + i
		const int* rows;  // (saves the kernel a dependent global load before it can touch the stream's state)
		int numStreams;
		int slot0, row0;
	};
	bool RecurrentDppSupported(const LstmModelDev& m);
	// four streams per wave (RecurrentQuadKernel) for launches of at least this many streams of LSTMs up to 2x16; tests / tuning
	bool RecurrentQuadSupported(const LstmModelDev& m);
	int RecurrentQuadMinStreams();
	int SetRecurrentQuadMinStreams(int streams); // returns the previous value
	long RecurrentQuadLaunches();
	hipError_t LaunchRecurrentDpp(const RecurrentGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride, int n,
		hipStream_t stream);
	// ... any number of groups in one launch, the group table in device memory (`table`: the batch's cache of it; wavenet_launch.h)
	struct WnLaunchTable;
	hipError_t LaunchRecurrentDppTable(const RecurrentGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride, int n,
		hipStream_t stream, WnLaunchTable& table);

	// state[k*capacity + slot] = init[k] for the listed slots
	hipError_t LaunchLstmInitState(float* state, int capacity, const int* slots, int numStreams, const float* init, int numElems,
		hipStream_t stream);

	// Pool re-arm: entry = member * 2 + prewarmed; state[k*capacity + member] = (prewarmed ? armed : init)[k] -- the armed state of a
	// recurrent model is the same for every stream, so one column per group (kept from a one-stream prewarm) serves them all
	hipError_t LaunchRecurrentRearm(float* state, int capacity, const int* entries, int numEntries, const float* init, const float* armed,
		int numElems, hipStream_t stream);
}
