// dvp_pyramid_run.h — the level images made on the device (dvp_pyramid.hip) as the engine's contexts use them.
#ifndef DVP_PYRAMID_RUN_H_
#define DVP_PYRAMID_RUN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"

namespace dvppyr {

// one decoded image on the device; a launch's images travel as a kernel argument
struct Source {
	const uint8_t* bytes;
	int sw, sh;
	long long pitch;
};
struct Sources { Source v[DVP_MAX_IMAGES]; };

int store_device(const dvp_images* store);
// the descriptors of ids[0 .. n-1], read under the store's lock; non-zero with *error set when an id is not in the store
int store_sources(const dvp_images* store, const int* ids, int n, Sources* out, std::string* error);
// for a slot that is filled on the device (dvp_jpeg_decode_into_store): whether `id` is in the store; and a finished w x h image (w bytes
// per row, nothing queued on it) joining the store under `id`, with dvp_images_put's accounting and its rule for an id that is
// there already — non-zero, and `bytes` stays with the caller
bool store_has(const dvp_images* store, int id);
int store_adopt(dvp_images* store, int id, dvpmem::DevBlock& bytes, int w, int h);
// Level lw x lh of images 0 .. n-1, each on a pad_w x pad_h canvas, into the planes interior + i * plane_stride (`pitch` floats per
// row) on `stream`: one launch, no host wait.  1 <= n <= DVP_MAX_IMAGES, every size >= 1, lh <= 262140.  Non-zero = the launch failed.
int launch_levels(hipStream_t stream, const Sources& images, int n, int pad_w, int pad_h, int lw, int lh, float* interior, int pitch, size_t plane_stride);

}   // namespace dvppyr
#endif
