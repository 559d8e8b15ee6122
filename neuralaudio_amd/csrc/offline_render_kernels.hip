// offline_render_kernels.hip -- the data movement of the offline renderer (offline_render.cpp): the gather that builds the segment
// rows of one pass from the signal windows of its jobs (zero past a job's end), and the scatter that moves the kept part of every
// segment row into the job's contiguous output (lead-ins and tail padding dropped).  The per-sample work runs on the batch engine's own
// kernels in between.
#include <hip/hip_runtime.h>

#include "offline_render.h"

namespace na
{
	// grid: x walks the row's frames, y = row
	__global__ void __launch_bounds__(256) RenderGatherKernel(const RenderRow* __restrict__ rows, const float* __restrict__ sig,
		float* __restrict__ buf, long long n)
	{
		const RenderRow r = rows[blockIdx.y];
		float* const dst = buf + (long long)blockIdx.y * n;
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
			dst[i] = i < r.valid ? sig[r.src + i] : 0.0f;
	}

	__global__ void __launch_bounds__(256) RenderScatterKernel(const RenderRow* __restrict__ rows, const float* __restrict__ buf,
		float* __restrict__ out, long long n)
	{
		const RenderRow r = rows[blockIdx.y];
		const float* const src = buf + (long long)blockIdx.y * n;
		const long long len = r.keepEnd - r.keepBegin;
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
			out[r.dst + i] = src[r.keepBegin + i];
	}

	namespace
	{
		dim3 RenderGrid(long long n, int numRows)
		{
			const long long blocks = (n + 255) / 256;
			return dim3((unsigned)(blocks < 1024 ? (blocks > 0 ? blocks : 1) : 1024), (unsigned)numRows);
		}
	}

	hipError_t LaunchRenderGather(const RenderRow* dRows, int numRows, const float* dSig, float* dBuf, long long n, hipStream_t stream)
	{
		if (numRows <= 0 || n <= 0) return hipSuccess;
		hipLaunchKernelGGL(RenderGatherKernel, RenderGrid(n, numRows), dim3(256), 0, stream, dRows, dSig, dBuf, n);
		return hipGetLastError();
	}

	hipError_t LaunchRenderScatter(const RenderRow* dRows, int numRows, const float* dBuf, float* dOut, long long n, hipStream_t stream)
	{
		if (numRows <= 0 || n <= 0) return hipSuccess;
		hipLaunchKernelGGL(RenderScatterKernel, RenderGrid(n, numRows), dim3(256), 0, stream, dRows, dBuf, dOut, n);
		return hipGetLastError();
	}
}
