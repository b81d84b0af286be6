// Host build of the device JPEG encoder's steps (dvp-mvs_amd/csrc/dvp_jpeg.hpp), one MCU and one restart segment after the
// other (TEST INFRASTRUCTURE): lets the CPU tests hold the encoder's arithmetic against libjpeg-turbo without a GPU.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_jpeg.hpp"

extern "C" int dvp_jpeg_encode_host(const uint8_t* pix, int W, int H, int C, long long pitch, int quality, int restart,
                                    uint8_t* dst, long long capacity, long long* bytes) {
	using namespace dvpjpeg;
	if (W < 1 || H < 1 || (C != 1 && C != 3) || restart < 1 || restart > 65535) return 1;
	Tables t;
	build_tables(quality, &t);
	const long long mcx = C == 3 ? (W + 15) / 16 : (W + 7) / 8, mcy = C == 3 ? (H + 15) / 16 : (H + 7) / 8;
	const int bpm = C == 3 ? 6 : 1;
	const long long nmcu = mcx * mcy;
	std::vector<int16_t> coef(nmcu * bpm * 64);
	std::vector<uint64_t> mask(nmcu * bpm);
	for (long long m = 0; m < nmcu; ++m) {
		if (C == 3) mcu_color(pix, pitch, W, H, (int)(m % mcx), (int)(m / mcx), &t, &coef[m * 384], &mask[m * 6]);
		else mcu_grey(pix, pitch, W, H, (int)(m % mcx), (int)(m / mcx), &t, &coef[m * 64], &mask[m]);
	}
	std::vector<uint8_t> out(1024);
	out.resize(build_header(&t, W, H, C, restart, out.data()));
	const long long nseg = (nmcu + restart - 1) / restart;
	for (long long s = 0; s < nseg; ++s) {
		const long long first = s * restart, n = first + restart <= nmcu ? restart : nmcu - first;
		CountOut cnt;
		code_segment(&t, coef.data(), mask.data(), first, n, bpm, cnt);
		const size_t at = out.size();
		out.resize(at + cnt.n);
		WriteOut wr{ out.data() + at };
		code_segment(&t, coef.data(), mask.data(), first, n, bpm, wr);
		if (s + 1 < nseg) { out.push_back(0xFF); out.push_back((uint8_t)(0xD0 + (s & 7))); }
	}
	out.push_back(0xFF); out.push_back(0xD9);
	*bytes = (long long)out.size();
	if ((long long)out.size() > capacity) return 2;
	memcpy(dst, out.data(), out.size());
	return 0;
}

// the device's preview renderers on the host: planes (x, y, z, w) + weak map -> three BGR images (NULL: skipped)
extern "C" void dvp_preview_render_host(const float* planes, const uint8_t* weak, long long L, float dmin, float dmax, uint8_t* depth_bgr,
                                        uint8_t* normal_bgr, uint8_t* weak_bgr) {
	using namespace dvpjpeg;
	for (long long i = 0; i < L; ++i) {
		const float* p = planes + 4 * i;
		const bool usable = !(p[3] < dmin || p[3] > dmax);
		if (depth_bgr) render_depth(usable ? p[3] : 0.0f, dmin, dmax, depth_bgr + 3 * i);
		if (normal_bgr) render_normal(p[0], p[1], p[2], normal_bgr + 3 * i);
		if (weak_bgr) render_weak(usable ? weak[i] : (uint8_t)2, weak_bgr + 3 * i);
	}
}
