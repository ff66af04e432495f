/*
 * hip_host.h — what the host side of the library does with the HIP runtime, once: the error macro, the device selection, the
 * owner of device allocations, the launch with dynamic LDS, the private stream; the overlap check of an entry's buffers comes with it
 * (buffers.h).  C++, for the units hipcc compiles only (the host-only units that the sanitizer builds compile with g++ do not see it).
 */
#ifndef MDEMOD_HIP_HOST_H
#define MDEMOD_HIP_HOST_H

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "buffers.h"
#include "mdemod_internal_api.h"

/* A hipError_t becomes the entry's return value: the text for mdemod_last_error(), the pending error dropped (it is reported: it
 * must not be read again as the status of somebody's next launch), out of memory told apart from everything else. */
#define HIP_TRY(expr)                                                                                  \
	do {                                                                                               \
		hipError_t e_ = (expr);                                                                        \
		if (e_ != hipSuccess) {                                                                        \
			mdm_note_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
			(void)hipGetLastError();                                                                   \
			return e_ == hipErrorOutOfMemory ? MDEMOD_ERR_NOMEM : MDEMOD_ERR_HIP;                      \
		}                                                                                              \
	} while (0)

/* Every device entry begins here.  The launch wrappers report hipGetLastError() after their launch: an error some EARLIER call of
 * this thread left behind (the caller's own, another library's, a refused hipSetDevice) would come back as the status of a launch
 * that went through (r06: a context made right after mdemod_create had refused a device that does not exist failed in
 * mdemod_launch_reset with that device's error).  A launch's status is the launch's: what is pending is dropped first. */
inline int
mdm_select_device(int device)
{
	(void)hipGetLastError();
	const hipError_t e = hipSetDevice(device);
	if (e != hipSuccess) {
		mdm_note_error("no usable HIP device %d: %s", device, hipGetErrorString(e));
		(void)hipGetLastError();
		return MDEMOD_ERR_HIP;
	}
	return MDEMOD_OK;
}

/* Device memory with one owner: everything it handed out is freed when it goes (a context's owner with the context, a call's with
 * the call).  The destroy functions select the device before that. */
struct MdmDevMem {
	std::vector<void *> blocks;
	MdmDevMem() = default;
	MdmDevMem(const MdmDevMem &) = delete;
	MdmDevMem &operator=(const MdmDevMem &) = delete;
	~MdmDevMem() { for (void *p : blocks) (void)hipFree(p); }

	/* One padding rule: 64 bytes behind `count` elements, and never less than one element.  The kernels' vector loads run up to
	 * 16 bytes past the last element they use (a row's tail, an empty table): that stays inside the allocation. */
	template <typename T>
	int alloc(T **out, size_t count)
	{
		void *p = nullptr;
		blocks.reserve(blocks.size() + 1);             /* (nothing can fail between the allocation and its entry in the list) */
		HIP_TRY(hipMalloc(&p, (count ? count : 1) * sizeof(T) + 64));
		blocks.push_back(p);
		*out = static_cast<T *>(p);
		return MDEMOD_OK;
	}

	/* one block back before the rest: buffers that are regrown */
	void release(void *p)
	{
		for (size_t i = 0; i < blocks.size(); i++)
			if (blocks[i] == p) { (void)hipFree(p); blocks.erase(blocks.begin() + i); return; }
	}
};

/* A stream of the call's own, destroyed on scope exit (the caller creates it: with flags, or with a priority). */
struct MdmStream {
	hipStream_t s = nullptr;
	MdmStream() = default;
	MdmStream(const MdmStream &) = delete;
	MdmStream &operator=(const MdmStream &) = delete;
	~MdmStream() { if (s) (void)hipStreamDestroy(s); }
};

/* A kernel with `lds` bytes of dynamic LDS: the attribute that allows more than 64 KB, the launch, the launch's status. */
template <typename... Params, typename... Args>
hipError_t
mdm_launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args &&... args)
{
	const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<Args>(args)...);
	return hipGetLastError();
}

#endif
