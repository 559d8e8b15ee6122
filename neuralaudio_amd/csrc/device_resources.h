// device_resources.h -- the HIP calls that create or release a device resource, counted (test build: NA_DebugDeviceResourceCalls).
// A real-time safe call of this library makes none of them: device and pinned allocations and frees, stream and event creations.  Every
// call site of the library goes through these wrappers, except the loopback stand-in for RCCL (rccl_loopback.cpp, test build), which
// plays the part of an outside library; the counter is process-wide.
#pragma once

#include <hip/hip_runtime_api.h>

namespace na
{
	void CountDeviceResourceCall();
	long long DeviceResourceCalls();

	template <typename... A> inline hipError_t CountedHipMalloc(A... a) { CountDeviceResourceCall(); return hipMalloc(a...); }
	template <typename... A> inline hipError_t CountedHipExtMallocWithFlags(A... a) { CountDeviceResourceCall(); return hipExtMallocWithFlags(a...); }
	template <typename... A> inline hipError_t CountedHipFree(A... a) { CountDeviceResourceCall(); return hipFree(a...); }
	template <typename... A> inline hipError_t CountedHipHostMalloc(A... a) { CountDeviceResourceCall(); return hipHostMalloc(a...); }
	template <typename... A> inline hipError_t CountedHipHostFree(A... a) { CountDeviceResourceCall(); return hipHostFree(a...); }
	template <typename... A> inline hipError_t CountedHipStreamCreateWithFlags(A... a) { CountDeviceResourceCall(); return hipStreamCreateWithFlags(a...); }
	template <typename... A> inline hipError_t CountedHipStreamCreate(A... a) { CountDeviceResourceCall(); return hipStreamCreate(a...); }
	template <typename... A> inline hipError_t CountedHipEventCreateWithFlags(A... a) { CountDeviceResourceCall(); return hipEventCreateWithFlags(a...); }
	template <typename... A> inline hipError_t CountedHipEventCreate(A... a) { CountDeviceResourceCall(); return hipEventCreate(a...); }
}
