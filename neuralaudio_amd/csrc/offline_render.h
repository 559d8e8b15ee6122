// offline_render.h -- time-parallel offline rendering of long signals (NA_RenderOffline, include/neuralaudio_amd.h).
//
// A WaveNet has no recurrence: output sample t depends only on the inputs in [t - H, t], H the summed history of the stream's rings.
// A long signal is cut into segments that run as the streams of one ordinary batch; segment g >= 1 starts `lead` >= H samples early
// from a prewarmed (or any earlier) state and keeps only the outputs after its lead-in, which are then the sequential run's bit for
// bit on the same kernel.  Recurrent models are not cut: each recurrent job is one stream, run sequentially.
#pragma once

#include <cstddef>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "model_loader.h"

namespace na
{
	// one row of a pass: the gather fills buf[row][0, n) from sig[src, src + valid) and zeros; the scatter copies buf[row][keepBegin,
	// keepEnd) to out[dst, dst + keepEnd - keepBegin).  Offsets are relative to the pass's device windows.
	struct RenderRow
	{
		long long src, valid;
		long long dst, keepBegin, keepEnd;
	};
	hipError_t LaunchRenderGather(const RenderRow* dRows, int numRows, const float* dSig, float* dBuf, long long n, hipStream_t stream);
	hipError_t LaunchRenderScatter(const RenderRow* dRows, int numRows, const float* dBuf, float* dOut, long long n, hipStream_t stream);

	struct RenderJobDesc
	{
		std::shared_ptr<const LoadedModel> model;
		float quality = 1.0f;
		const float* input = nullptr;
		float* output = nullptr;
		size_t numSamples = 0;
	};

	struct RenderOptionsDesc
	{
		size_t segmentSamples = 0;    // 0: the planner's choice
		size_t maxSamplesPerPass = 0; // 0: kDefaultMaxSamplesPerPass
		double waitLimitMs = 0.0;     // 0: the batch default (NA_WAIT_LIMIT_MS / 2000 ms)
	};

	constexpr size_t kDefaultMaxSamplesPerPass = (size_t)1 << 26; // 64 Mi samples: 256 MB of segment rows
	constexpr int kMaxRenderRows = 16384;

	// the summed history of the rings the stream's plan keeps (wavenet_plan.cpp AddRing: one ring of (K - 1) d frames per conv layer, one
	// of (K - 1) d for a conv head), dilations after oversampling; -1 for a recurrent model
	int StreamHistory(const LoadedModel& model, float quality);

	struct RenderPlan
	{
		int lead = 0;              // lead-in of every segment after the first (a multiple of 128; 0 without WaveNet jobs)
		long long rowSamples = 0;  // n: frames every row processes per pass
		long long stride = 0;      // L = n - lead: segment g >= 1 of a WaveNet job reads [g L, g L + n) and keeps [g L + lead, ..)
		int passes = 0;
		int rows = 0;              // streams of the segment batch
		long long segments = 0;    // segments over all jobs (a recurrent job: 1)
		double estimatedMs = 0.0;  // the cost model's estimate of the device time
		std::vector<int> jobRows;  // per job: rows of the batch (0: an empty job)
		std::vector<long long> jobSegments;
		std::vector<char> jobRecurrent;
	};

	// `computeUnits` <= 0: the MI355X's 256
	RenderPlan PlanOfflineRender(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int computeUnits);
	// the plan of `jobs` on `device`'s compute units (256 without a device); kernelName: the kernel of job 0's first segment row when a
	// device is present (a batch of the plan's rows is built for the question), else ""
	RenderPlan PlanOfflineRenderOn(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, std::string* kernelName);
	// renders every job on `device`; throws std::runtime_error / HipError with the reason (no device, a wait that ran into the limit, ...)
	void RenderOffline(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device);

	// ---- the same at an external sample rate (NA_RenderOfflineAtRate): every job's input / output / numSamples are at `externalRate`,
	// its model runs at its own LoadedModel::ProcessRate().  Per job: plan = PlanResampling(externalRate, model rate, quantum 1),
	// L = plan.latency, M = J(N + L) model frames; x is uploaded whole, the up stage (offline_resample_kernels.hip) makes u[0, M), the
	// segment machinery above renders u -> v with both in device memory, the down stage makes out[k] = s[k + L], downloaded whole.
	// An identity pair skips both stages (u = x, out = v): RenderOffline's result.  Device memory on top of RenderOffline's: 8 N + 8 M
	// bytes per job (8 M for an identity job) plus the coefficient tables.  Refusals (a rate <= 0, a refused pair, overlapping buffers)
	// come before any device work.
	struct ResamplePlan;
	// segmentSamples / maxSamplesPerPass and every figure of the plan count MODEL-RATE frames; firstJobPlan: job 0's resampling plan
	RenderPlan PlanOfflineRenderAtRateOn(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, int externalRate,
		std::string* kernelName, ResamplePlan* firstJobPlan);
	void RenderOfflineAtRate(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, int externalRate);
	// tests (NA_DebugSetRenderTap): the next RenderOfflineAtRate copies job 0's u and v (M frames each) to these host arrays and fails
	// before any device work if M > capacity; both NULL: off.  One call only.
	void SetRenderTap(float* modelIn, float* modelOut, long long capacity);
}
