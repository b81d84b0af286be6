// REFERENCE PIN — TEST INFRASTRUCTURE ONLY.
// Stand-in for the CUDA headers main.h includes, so that the device part of the reference's APD.cu
// (everything in front of APD::RunPatchMatch) compiles unchanged with g++ and runs on the host.
// Only what that text uses: the vector types, empty qualifiers, the thread indices, tex2D<float>,
// the three cuRAND calls, rsqrtf and CUDA's float min/max.  Written from the CUDA C++ Programming
// Guide; it shares no code with oracle/ora_core.h on purpose — the pin test compares the two
// statements of the texture unit.
#ifndef DVP_REF_SHIM_CUDA_RUNTIME_H_
#define DVP_REF_SHIM_CUDA_RUNTIME_H_

#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct short2 { short x, y; };
struct uint3 { unsigned x, y, z; };
struct dim3 { unsigned x = 1, y = 1, z = 1; };
// CUDA's make_* take the element type: an int or float argument to make_short2 converts implicitly
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
inline short2 make_short2(short x, short y) { return short2{x, y}; }

typedef int cudaError_t;
struct cudaArray;
typedef unsigned long long cudaTextureObject_t;

// thread indices: set by the harness's launch loop (ref_harness.cpp), one thread at a time
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

// ---- texture unit ------------------------------------------------------------------------------
// A texture object is the address of one of these.  The reference creates every image and depth
// texture with cudaFilterModeLinear, cudaReadModeElementType, normalizedCoords = 0 and
// cudaAddressModeWrap (APD.cpp:1509-1516, 1534-1541).  With unnormalised coordinates wrap is not
// available and the runtime switches to cudaAddressModeClamp (CUDA Runtime API, cudaTextureDesc:
// "if normalizedCoords is zero, Wrap and Mirror won't be supported and will be switched to Clamp").
struct RefTexture { const float* data; int width, height; };
extern int dvp_ref_sampler;   // 0: the Guide's 8-bit fixed-point fractions; 1: exact fractions (ours)

// Programming Guide, "Texture Fetching / Linear Filtering", 2-D:
//   tex(x, y) = (1-a)(1-b) T[i,j] + a(1-b) T[i+1,j] + (1-a) b T[i,j+1] + a b T[i+1,j+1]
//   xB = x - 0.5, i = floor(xB), a = frac(xB) stored in 9-bit fixed point with 8 bits of fraction;
//   clamp addressing: an index outside [0, N-1] reads the border texel of that side.
// The weighted sum is evaluated as two horizontal lerps and one vertical lerp, each as one fused
// multiply-add t0 + a (t1 - t0) (the hardware's internal precision is not specified; this choice is
// the oracle contract's too and is one of the things this pin does NOT establish).
inline int dvp_ref_clamp_index(float f, int n) {
	if (!(f > -2.0f)) return 0;               // also NaN
	if (f > (float)n) return n - 1;
	const int i = (int)f;
	return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
inline float dvp_ref_tex_fetch(const RefTexture* t, float x, float y) {
	// coordinates far outside read the border texel whatever the fraction: clamp them first so the
	// float -> int conversion below is defined (NaN reads texel 0 with fraction 0)
	float xb = x - 0.5f, yb = y - 0.5f;
	if (!(xb > -1.0f)) xb = -1.0f;
	if (xb > (float)t->width) xb = (float)t->width;
	if (!(yb > -1.0f)) yb = -1.0f;
	if (yb > (float)t->height) yb = (float)t->height;
	const float fi = floorf(xb), fj = floorf(yb);
	float a = xb - fi, b = yb - fj;
	if (dvp_ref_sampler == 0) {
		a = floorf(a * 256.0f + 0.5f) / 256.0f;   // 8 fractional bits, round to nearest (1.0 representable)
		b = floorf(b * 256.0f + 0.5f) / 256.0f;
	}
	const int i0 = dvp_ref_clamp_index(fi, t->width), i1 = dvp_ref_clamp_index(fi + 1.0f, t->width);
	const int j0 = dvp_ref_clamp_index(fj, t->height), j1 = dvp_ref_clamp_index(fj + 1.0f, t->height);
	const float t00 = t->data[j0 * t->width + i0], t10 = t->data[j0 * t->width + i1];
	const float t01 = t->data[j1 * t->width + i0], t11 = t->data[j1 * t->width + i1];
	const float r0 = fmaf(a, t10 - t00, t00);
	const float r1 = fmaf(a, t11 - t01, t01);
	return fmaf(b, r1 - r0, r0);
}
template <class T>
inline T tex2D(cudaTextureObject_t obj, float x, float y) {
	return (T)dvp_ref_tex_fetch((const RefTexture*)(uintptr_t)obj, x, y);
}

// ---- cuRAND ------------------------------------------------------------------------------------
// The reference hands one curandState to every sampling site; the oracle gives each logical site a
// counter-based sub-stream.  The call site's source line picks the sub-stream (oracle/ref_draws.json
// through the harness); curand_init does nothing.
struct curandState { int unused; };
float dvp_ref_uniform(int line);
unsigned dvp_ref_u32(int line);
#define curand_uniform(state) dvp_ref_uniform(__LINE__)
#define curand(state) dvp_ref_u32(__LINE__)
#define curand_init(seed, sequence, offset, state) ((void)0)
inline long long clock64() { return 0; }

// ---- math -----------------------------------------------------------------------------------------
// CUDA's math API overloads the C names in the global namespace: exp(float) IS expf, sqrt(float) IS
// sqrtf, and a double argument picks the double function.  C++'s <math.h> does the same; <cmath> alone
// leaves only the double functions there, and exp(float) would quietly run in double.
#include <math.h>
using std::isnan;
// oracle contract list (ora_common.h): rsqrtf(x) = 1.0f / sqrtf(x); float min/max are CUDA's
// NaN-ignoring fminf/fmaxf; integer min/max are the usual ones.
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }

#endif
