// dvp_viewclean_run.h — the visibility-mask clean-up on the device (dvp_viewclean.hip) as the engine's contexts use it.
#ifndef DVP_VIEWCLEAN_RUN_H_
#define DVP_VIEWCLEAN_RUN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvp_devmem.hpp"
#include "dvp_viewclean.hpp"

namespace dvpvc {

// Device scratch: per bit plane and pixel one parent word and one size word (8 * planes bytes per pixel, one allocation); grows,
// and is kept for the next map that needs no more.
struct Scratch {
	dvpmem::DevBlock block;      // [planes][L] parent words, then [planes][L] size words
	unsigned* words() const { return block.as<unsigned>(); }
};
int scratch_reserve(Scratch& s, size_t pixels, int planes);   // non-zero: out of device memory
void scratch_free(Scratch& s);

// views -> out (W * H words each, out == views is allowed) on `stream`: four launches (one when num_src == 0) whatever the
// words hold, no host wait; 0 <= num_src <= 32, W * H < 2^31, s reserved for (W * H, num_src).  Non-zero = a launch failed.
int launch_clean(hipStream_t stream, Scratch& s, const uint32_t* views, int W, int H, int num_src, int min_region, uint32_t* out);
// The first three of those launches alone (the label prior's components, dvp_labels.hip): afterwards, per plane b, the words
// s.words() + b * L lead every clear pixel to its component's root — the component's smallest pixel index — and the words
// s.words() + (num_src + b) * L hold the component's size at the root.
int launch_components(hipStream_t stream, Scratch& s, const uint32_t* views, int W, int H, int num_src);

}   // namespace dvpvc
#endif
