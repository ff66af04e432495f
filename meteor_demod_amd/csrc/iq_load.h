/*
 * iq_load.h — one IQ sample of a recording as a float pair, for the kernels that read single samples (front end, survey).
 * The demodulator kernels and the recording estimators have loaders of their own: they load several samples at a time.
 */
#ifndef MDEMOD_IQ_LOAD_H
#define MDEMOD_IQ_LOAD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* FMT: bits per component; 8: unsigned, offset 128; 16: signed; 32: float */
template <int FMT>
__device__ __forceinline__ float2
md_load_iq(const void *iq, uint64_t i)
{
	if (FMT == 8) {
		const uchar2 v = static_cast<const uchar2 *>(iq)[i];
		return make_float2(static_cast<float>(static_cast<int>(v.x) - 128), static_cast<float>(static_cast<int>(v.y) - 128));
	} else if (FMT == 16) {
		const short2 v = static_cast<const short2 *>(iq)[i];
		return make_float2(static_cast<float>(v.x), static_cast<float>(v.y));
	} else {
		return static_cast<const float2 *>(iq)[i];
	}
}

#endif
