// dvp_jpeg_dec.hpp — the arithmetic of the input JPEG decoder that is independent per block and per pixel, as __host__ __device__
// functions: the host mirror (host/jpeg.cpp) runs them block after block and pixel after pixel, the kernels of dvp_jpeg_dec.hip a
// lane per column / row / pixel.  One text, one result.
//   block   coefficient records (dvp_jpeg_dec_mid.hpp) -> dequantised coefficients -> accurate integer inverse DCT
//           (Loeffler-Ligtenberg-Moschytz, 13-bit constants, 2 guard bits: libjpeg's "islow") -> + 128, clamp
//   pixel   replicated chroma sample at (y * v / vmax, x * h / hmax); the three JFIF equations in binary64, one rounding per
//           operator (build with -ffp-contract=off), lround, clamp; B, G, R
// All products and sums of the transform are 64-bit, as the dense decoder's were: a 16-bit quantiser times a 16-bit value is up to
// 2^31, times a 14-bit constant and summed over eight terms it is far past 32 bits, and nothing in a file bounds it.  There is no
// narrower path.
#ifndef DVP_JPEG_DEC_HPP_
#define DVP_JPEG_DEC_HPP_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DVP_JD_HD __host__ __device__
#else
#define DVP_JD_HD
#endif

namespace dvpjd {

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819,
              F2562 = 20995, F3072 = 25172;

struct QTable { uint16_t q[64]; };   // natural order; travels to a kernel as an argument

DVP_JD_HD inline int record_position(uint32_t record) { return (int)(record & 63u); }
DVP_JD_HD inline int record_value(uint32_t record) { return (int)record >> 6; }   // (arithmetic shift: the sign comes down with it)
// the dequantised coefficient of a record (the dense decoder's `int coef = value * q`)
DVP_JD_HD inline int dequantised(uint32_t record, const uint16_t* q) { return (int)((long long)record_value(record) * (long long)q[record_position(record)]); }

DVP_JD_HD inline int descale(long long x, int n) { return (int)((x + (1LL << (n - 1))) >> n); }

// One 1-D pass over eight values, the same for both directions: a column of coefficients, still to be descaled by CONST_BITS -
// PASS1_BITS into the workspace, or a workspace row, still to be descaled by CONST_BITS + PASS1_BITS + 3.  out[k] is sample k.
DVP_JD_HD inline void idct_line(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, long long out[8]) {
	long long z2 = i2, z3 = i6;
	long long z1 = (z2 + z3) * F0541;
	long long tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
	long long tmp0 = ((long long)i0 + i4) * (1LL << CONST_BITS), tmp1 = ((long long)i0 - i4) * (1LL << CONST_BITS);   // (a shift, for negative values too)
	const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
	tmp0 = i7; tmp1 = i5; tmp2 = i3; tmp3 = i1;
	z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
	long long z4 = tmp1 + tmp3;
	const long long z5 = (z3 + z4) * F1175;
	tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
	z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
	z3 += z5; z4 += z5;
	tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
	out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
	out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
	out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
	out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// column c of a block: coef[r * stride + c] (dequantised, natural order) -> ws[r * stride + c].  In place is fine: a column
// reads all of its eight values before it writes, and no other column's.
DVP_JD_HD inline void idct_column(const int* coef, int* ws, int stride, int c) {
	long long o[8];
	const int* p = coef + c;
	idct_line(p[0], p[stride], p[2 * stride], p[3 * stride], p[4 * stride], p[5 * stride], p[6 * stride], p[7 * stride], o);
	for (int r = 0; r < 8; ++r) ws[r * stride + c] = descale(o[r], CONST_BITS - PASS1_BITS);
}

DVP_JD_HD inline uint8_t clamp_sample(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// row r of a block: ws[r * stride + 0 ... 7] -> eight samples
DVP_JD_HD inline void idct_row(const int* ws, int stride, int r, uint8_t out[8]) {
	long long o[8];
	const int* p = ws + r * stride;
	idct_line(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], o);
	for (int c = 0; c < 8; ++c) out[c] = clamp_sample(descale(o[c], CONST_BITS + PASS1_BITS + 3) + 128);
}

// the records of one block -> 64 dequantised coefficients, natural order, row stride 8
DVP_JD_HD inline void densify(const uint32_t* records, uint32_t count, const uint16_t* q, int coef[64]) {
	for (int i = 0; i < 64; ++i) coef[i] = 0;
	for (uint32_t k = 0; k < count; ++k) coef[record_position(records[k])] = dequantised(records[k], q);
}

// one whole block, serially: records -> 8 x 8 samples at out (row pitch `pitch` bytes)
DVP_JD_HD inline void reconstruct_block(const uint32_t* records, uint32_t count, const uint16_t* q, uint8_t* out, size_t pitch) {
	int ws[64];
	densify(records, count, q, ws);
	for (int c = 0; c < 8; ++c) idct_column(ws, ws, 8, c);
	for (int r = 0; r < 8; ++r) idct_row(ws, 8, r, out + (size_t)r * pitch);
}

// where pixel (x, y) of the image samples a component plane with sampling factors (h, v) out of (hmax, vmax): replicated, no
// interpolation
DVP_JD_HD inline int sample_row(int y, int v, int vmax) { return y * v / vmax; }
DVP_JD_HD inline int sample_col(int x, int h, int hmax) { return x * h / hmax; }

// JFIF YCbCr -> B, G, R
DVP_JD_HD inline void ycc_to_bgr(int yy, int cb_sample, int cr_sample, uint8_t bgr[3]) {
	const int cb = cb_sample - 128, cr = cr_sample - 128;
	const int r = (int)lround(yy + 1.402 * cr);
	const int g = (int)lround(yy - 0.344136 * cb - 0.714136 * cr);
	const int b = (int)lround(yy + 1.772 * cb);
	bgr[0] = clamp_sample(b);
	bgr[1] = clamp_sample(g);
	bgr[2] = clamp_sample(r);
}

}   // namespace dvpjd
#endif
