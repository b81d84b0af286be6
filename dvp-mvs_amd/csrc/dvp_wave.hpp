// dvp_wave.hpp — what the wave-per-pixel kernels of every launch-site family share: the lane sections and the
// shared-memory helpers of one wavefront.
//
// Code shape.  A wave runs a `*_wave` function in lock step.  `DVP_LANES(l) { ... }` marks a section in which lane l does
// its own share (on the device: the calling lane; in the host emulation of tests/emul: a loop over 64 lanes); everything
// outside such sections is per-pixel ("uniform") code that every lane executes with identical values, writing shared state
// only from lane 0 (`DVP_LANE0`).  wave_sync() orders shared-memory traffic between sections.  The reference has no such
// code: it runs one thread per pixel throughout (APD.cu:3091-3165).
// The bit helpers that only the weak update uses stay with it: nth_set_bit (dvp_weak_wave.hpp), wave_lane_bit (dvp_weak_phased.hpp).
#ifndef DVP_WAVE_HPP_
#define DVP_WAVE_HPP_

#include "dvp_dev.hpp"

namespace dvp {

#if defined(__HIP_DEVICE_COMPILE__)
#define DVP_LANES(L) for (int L = (int)(threadIdx.x & 63u), once_##L = 1; once_##L; once_##L = 0)
#define DVP_LANE0 ((threadIdx.x & 63u) == 0u)
DVP_HD void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#else
#define DVP_LANES(L) for (int L = 0; L < 64; ++L)
#define DVP_LANE0 true
DVP_HD void wave_sync() {}
#endif

// shared-memory counters / bit sets touched by several lanes of the wave in one section
DVP_HD int wave_counter_add(int* counter) {
#if defined(__HIP_DEVICE_COMPILE__)
	return atomicAdd(counter, 1);
#else
	return (*counter)++;
#endif
}
// Slot of the calling lane in a list that the lanes with `pred` append to IN LANE ORDER; *counter (shared memory) is the
// list length.  Every lane of the wave must call it (no early exit before it inside the section).
DVP_HD int wave_ordered_slot(bool pred, int* counter) {
#if defined(__HIP_DEVICE_COMPILE__)
	const unsigned long long m = __ballot(pred);
	const int base = *counter;
	const unsigned lane = threadIdx.x & 63u;
	wave_sync();
	if (lane == 0) *counter = base + __popcll(m);
	return base + __popcll(m & ((1ull << lane) - 1ull));
#else
	const int r = *counter;
	if (pred) (*counter)++;
	return r;
#endif
}
DVP_HD void wave_bits_or(uint32_t* word, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
	atomicOr(word, bits);
#else
	*word |= bits;
#endif
}

}  // namespace dvp
#endif
