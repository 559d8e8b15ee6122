// resample.h -- batch resampling between an external (host) sample rate and the model-side rate.
//
// The reference has no counterpart: it serves whole multiples of the model's rate by multiplying the dilations (NeuralModel.cpp:92-114,
// model_loader.cpp OversampleFactor) and leaves every other rate to the host.  Here a batch is ONE clock domain: one external rate Fe,
// one model rate Fm, one phase for all its streams.  With Fc = lcm(Fe, Fm), te = Fc / Fe and tm = Fc / Fm ticks per sample, one
// Kaiser-windowed sinc prototype h at Fc (length K = 48 * max(te, tm) + 1) serves both directions:
//   up    u[j]   = te * sum_i x[i] * h[j * tm - i * te]              (external -> model)
//   down  out[k] = tm * sum_j v[j] * h[k * te - S - j * tm]          (model -> external)
// The model only ever runs whole multiples of the block quantum q: after E external samples it has run P(E) = floor(J(E) / q) * q frames,
// J(E) = floor((E - 1) * te / tm) + 1 the frames the up stage can compute.  S = (q - 1) * tm + pad makes every v[j] an output needs
// available and the latency (48 * max(te, tm) + S) / te a whole number of external samples.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

namespace na
{
	constexpr int kResampleT = 48;          // prototype length in samples of the lower rate
	constexpr int kResampleMaxTicks = 640;  // te, tm beyond this are refused
	constexpr int kResampleDefaultQuantum = 32;

	struct ResamplePlan
	{
		int externalRate = 0, modelRate = 0;
		int te = 1, tm = 1;
		int tapsUp = 0, tapsDown = 0;
		int quantum = 1;
		int shift = 0;       // S, ticks
		int latency = 0;     // external samples
		int K = 0;           // prototype length
		bool identity = true; // equal rates: nothing runs
		// history lengths (samples kept per stream between calls): the up stage's external-rate inputs, the down stage's model-rate outputs
		int histUp = 0, histDown = 0;

		long long ComputableFrames(long long E) const { return E <= 0 ? 0 : ((E - 1) * te) / tm + 1; } // J(E)
		long long ModelFrames(long long E) const { return identity ? E : (ComputableFrames(E) / quantum) * quantum; } // P(E)
	};

	// throws std::runtime_error naming the reason (rate <= 0, a quantum other than 0 / 1 / 32 / 64 / 128, reduced terms beyond 640)
	ResamplePlan PlanResampling(int externalRate, int modelRate, int quantum);
	// a model that runs at `modelProcessRate` as loaded does not belong in a batch that resamples to `planModelRate`: throws (the one
	// message of NA_BatchAddStreams and NA_MultiAddStreams)
	void CheckResampleModelRate(int modelProcessRate, int planModelRate);
	// the prototype of a rate pair: designed in double precision, rounded to f32 once
	std::vector<float> ResamplePrototype(const ResamplePlan& plan);
	// phase-major coefficient tables of the two stages: up[phase][tap] = h[phase + tap * te] (te phases, tapsUp taps), down[phase][tap] =
	// h[phase + tap * tm] (tm phases, tapsDown taps); entries beyond the prototype are 0
	void ResampleTables(const ResamplePlan& plan, const std::vector<float>& h, std::vector<float>& up, std::vector<float>& down);

	// One launch per stage for the whole batch, one workgroup per row (resample_kernels.hip).  `hist` rows are `histLen` floats apart and
	// hold the last histLen samples before this call; the kernel replaces them with the last histLen of (history ++ this call's samples).
	// Output o reads the window (history ++ samples) at index (tick0 + o * step) / period - tap with the coefficients of phase
	// (tick0 + o * step) % period; the caller guarantees that every index lies inside the window.
	struct ResampleStageArgs
	{
		const float* in;   // rows inStride apart, nIn samples each (NaN reads as 0 when cleanNaN)
		float* out;        // rows outStride apart, nOut samples each
		long inStride, outStride;
		float* hist;
		const float* table; // [period][taps]
		int rows, nIn, nOut, histLen, taps;
		int tick0, step, period;
		float gain;
		int cleanNaN;
	};
	hipError_t LaunchResampleUp(const ResampleStageArgs& a, hipStream_t stream);
	hipError_t LaunchResampleDown(const ResampleStageArgs& a, hipStream_t stream);
	constexpr int kResampleWindowFloats = 12288; // LDS window of a workgroup: history + the samples of one piece (48 KiB)

	// ---- whole-signal stages of NA_RenderOfflineAtRate (offline_resample_kernels.hip): the same sums over a signal of any length.
	// One workgroup computes `tile` consecutive outputs of one job from a window of the job's input that it stages once in LDS (zero
	// outside [0, nIn)).  Output o's newest tap sits at tick tick0 + o * step (64-bit: two hours at 44.1 kHz are 5e10 ticks); it reads
	// the input at tick / period - tap with the coefficients of phase tick % period, exactly as ResampleStageArgs describes.
	struct OfflineResampleJob
	{
		const float* in;    // nIn samples (device)
		float* out;         // nOut samples (device)
		const float* table; // [period][taps] (device)
		long long nIn, nOut;
		long long tick0;    // >= 0
		int step, period, taps;
		int tile;           // outputs per workgroup (OfflineResampleTile)
		int window;         // floats a workgroup stages (OfflineResampleWindow of the tile)
		float gain;
	};
	constexpr int kOfflineResampleTile = 2048;       // the largest tile; 8 outputs per thread
	constexpr int kOfflineResampleWindowFloats = 12288;
	// floats a tile of `tile` outputs stages: taps + floor((period - 1 + (tile - 1) * step) / period), the span from the oldest tap of its
	// first output to the newest tap of its last one at the worst phase of the first
	long long OfflineResampleWindow(int tile, int step, int period, int taps);
	// the largest power of two <= kOfflineResampleTile whose window fits kOfflineResampleWindowFloats; 0 if not even one output does
	int OfflineResampleTile(int step, int period, int taps);
	// `jobs` (host copy) and `dJobs` (the same array in device memory, already enqueued on `stream`) describe numJobs jobs; the launcher
	// checks every job's integers -- the window indices its kernel will form -- before it launches one grid of (tiles, jobs)
	hipError_t LaunchOfflineResampleUp(const OfflineResampleJob* jobs, const OfflineResampleJob* dJobs, int numJobs, hipStream_t stream);
	hipError_t LaunchOfflineResampleDown(const OfflineResampleJob* jobs, const OfflineResampleJob* dJobs, int numJobs, hipStream_t stream);
}
