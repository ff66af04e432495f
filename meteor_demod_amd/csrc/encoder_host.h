/*
 * encoder_host.h — what the host models of the two encoders (csrc/jpeg_host.cpp, csrc/png_host.cpp) share.  Free of the GPU runtime.
 */
#ifndef MDEMOD_ENCODER_HOST_H
#define MDEMOD_ENCODER_HOST_H

#include <cstring>
#include <vector>

#include "mdemod_internal_api.h"

/* the model's file to the caller: its size always, its bytes when they fit */
inline int
enc_give(const char *who, const std::vector<uint8_t> &file, uint8_t *out, uint64_t out_room, uint64_t *bytes)
{
	if (bytes) *bytes = file.size();
	if (file.size() > out_room) {
		mdm_note_error("%s: the output needs %llu bytes, out_room is %llu", who, static_cast<unsigned long long>(file.size()), static_cast<unsigned long long>(out_room));
		return MDEMOD_ERR_OVERFLOW;
	}
	if (!file.empty()) memcpy(out, file.data(), file.size());
	return MDEMOD_OK;
}

#endif
