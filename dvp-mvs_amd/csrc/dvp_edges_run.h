// dvp_edges_run.h — the device Canny edge prior (dvp_edges.hip) as the engine's contexts use it.
#ifndef DVP_EDGES_RUN_H_
#define DVP_EDGES_RUN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvp_devmem.hpp"
#include "dvp_edges.hpp"

namespace dvpedge {

// parent words are read and written by other CUs inside the same launch: device-scope atomics (L2), never L1
struct DevMem {
	__host__ __device__ unsigned load(const unsigned* p) const {
#if defined(__HIP_DEVICE_COMPILE__)
		return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		return *p;
#endif
	}
	__host__ __device__ unsigned min(unsigned* p, unsigned v) const {
#if defined(__HIP_DEVICE_COMPILE__)
		return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
		const unsigned o = *p;
		if (v < o) *p = v;
		return o;
#endif
	}
};

// Device scratch of one map, 7 bytes per pixel (+ 1 per output map the caller keeps) in one block; grows, and is kept for the next
// map of the same or a smaller size.
struct Scratch {
	dvpmem::DevBlock block;
	// the block's parts
	uint8_t* grey = nullptr;     // [L] grey bytes; after the suppression has read them: the 0 / 255 map before the fix-ups
	uint8_t* map3 = nullptr;     // [L] 0 = candidate, 1 = nothing, 2 = strong
	uint8_t* mark = nullptr;     // [L] mark[root] = the set holds a strong pixel
	unsigned* parent = nullptr;  // [L] union-find links
	unsigned* hist = nullptr;    // [256] grey histogram, then [256] = low, [257] = high (as int)
};
int scratch_reserve(Scratch& s, size_t pixels);   // non-zero: out of device memory
void scratch_free(Scratch& s);

// Every launch_* below issues a fixed number of launches on `stream` and never waits; non-zero = a launch failed.
// stage 1 from a float plane: element (x, y) at src[(y * pitch + x) * step]  -> s.grey, and its histogram
int launch_grey_from_float(hipStream_t stream, Scratch& s, const float* src, long long pitch, int step, int W, int H);
// stages 2-4 from s.grey -> s.map3 (thresholds stay in s.hist); have_hist: launch_grey_from_float made the histogram already
int launch_suppress(hipStream_t stream, Scratch& s, int W, int H, bool have_hist);
// stage 5 from s.map3 -> s.grey (0 / 255, no fix-ups)
int launch_hysteresis(hipStream_t stream, Scratch& s, int W, int H);
// stage 6 from s.grey -> out (and out2 unless NULL)
int launch_fixups(hipStream_t stream, Scratch& s, int W, int H, uint8_t* out, uint8_t* out2);

}   // namespace dvpedge
#endif
