/*
 * frames_link.hip — the GPU entries of the link variant of the frame layer (include/meteor_demod_amd_frames_link.h).  The kernels
 * and the pipelines are those of csrc/frames.hip under a mode (csrc/frames_device.h); with both switches off every entry hands on
 * to the one without `_link`.
 */
#include "frames_device.h"
#include "hip_host.h"

extern "C" {

int
mdemod_frames_link_candidates_device(const mdemod_frames_link *link, const int8_t *soft_dev, uint64_t m, mdemod_frames_candidate *cand_dev, int device,
                                     void *hip_stream)
try { MDEMOD_API_ENTER
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_candidates_device(soft_dev, m, cand_dev, device, hip_stream);
	if (!fr_mode_windows(m, md)) return MDEMOD_OK;
	if (!soft_dev || !cand_dev) REFUSE("mdemod_frames_link_candidates_device: the symbols and the candidates are needed");
	rc = mdm_select_device(device);
	if (rc) return rc;
	return fr_candidates_run(md, soft_dev, m, cand_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_link_viterbi_device(const mdemod_frames_link *link, const int8_t *soft_dev, uint64_t m, mdemod_frame_info *frames, uint64_t n_frames,
                                  uint8_t *cadu_dev, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_viterbi_device(soft_dev, m, frames, n_frames, cadu_dev, device, hip_stream);
	if (!n_frames) return MDEMOD_OK;
	if (!soft_dev || !frames || !cadu_dev) REFUSE("mdemod_frames_link_viterbi_device: the symbols, the frames and the output are needed");
	rc = fr_check_frames(frames, n_frames, m, md);
	if (rc) return rc;
	rc = mdm_select_device(device);
	if (rc) return rc;
	return fr_viterbi_run(md, soft_dev, m, frames, n_frames, cadu_dev, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_link_decode_device(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft_dev, uint64_t m, uint8_t *cadu,
                                 mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device, void *hip_stream)
try { MDEMOD_API_ENTER
	if (n_frames) *n_frames = 0;
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_decode_device(opts, soft_dev, m, cadu, frames, cap, n_frames, device, hip_stream);
	if (!n_frames || (m && !soft_dev) || (cap && (!frames || !cadu)))
		REFUSE("mdemod_frames_link_decode_device: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	rc = fr_settings(opts, o);
	if (rc) return rc;
	return fr_decode_device(md, o, soft_dev, m, cadu, frames, cap, n_frames, device, static_cast<hipStream_t>(hip_stream));
} MDEMOD_API_CATCH

int
mdemod_frames_link_decode_host(const mdemod_frames_link *link, const mdemod_frames_opts *opts, const int8_t *soft, uint64_t m, uint8_t *cadu,
                               mdemod_frame_info *frames, uint64_t cap, uint64_t *n_frames, int device)
try { MDEMOD_API_ENTER
	if (n_frames) *n_frames = 0;
	FrMode md;
	int rc = fr_mode_of(link, md);
	if (rc) return rc;
	if (fr_mode_plain(md)) return mdemod_frames_decode_host(opts, soft, m, cadu, frames, cap, n_frames, device);
	if (!n_frames || (m && !soft) || (cap && (!frames || !cadu)))
		REFUSE("mdemod_frames_link_decode_host: the symbols, n_frames (and the outputs for cap > 0) are needed");
	*n_frames = 0;
	mdemod_frames_opts o;
	rc = fr_settings(opts, o);
	if (rc) return rc;
	return fr_decode_host(md, o, soft, m, cadu, frames, cap, n_frames, device);
} MDEMOD_API_CATCH

} /* extern "C" */
