// jpeg.cpp — baseline / extended-sequential JPEG decoder (8-bit, Huffman), so that a dense folder written
// by the reference's converter (colmap2mvsnet.py:424-469: images/%08d.jpg) is consumable as is.  Replaces
// cv::imread (APD.cpp:1057, 1842), which sits on libjpeg.
//
// Grey output is what libjpeg delivers for JCS_GRAYSCALE (OpenCV's IMREAD_GRAYSCALE on a JPEG): the luma
// plane, reconstructed with the accurate integer inverse DCT (Loeffler-Ligtenberg-Moschytz, 13-bit
// constants, 2 guard bits — libjpeg's default "islow" method).  tests/test_boundary.py pins it bit for
// bit against this image's own libjpeg (through PIL, draft mode 'L').  Colour output (fusion only:
// point colours) replicates chroma samples and uses the JFIF YCbCr -> RGB equations; libjpeg's default
// "fancy" chroma interpolation is not reproduced, colours at chroma edges can differ by a few levels.
// Progressive, lossless, arithmetic-coded and 12-bit files are rejected (empty Mat + message).
//
// The decoder's text is shared with the engine library (`apd --decode-on gpu`): the marker parse and the entropy decode are
// csrc/dvp_jpeg_dec_mid.hpp, which leaves coefficient records; the block and pixel arithmetic is csrc/dvp_jpeg_dec.hpp, run here
// serially and by the kernels of csrc/dvp_jpeg_dec.hip on the device.
#include "APD.h"
#include <cstdio>
#include "../csrc/dvp_jpeg_dec.hpp"
#include "../csrc/dvp_jpeg_dec_mid.hpp"

namespace {

bool read_file(const path& p, std::vector<uint8_t>* out) {
	FILE* f = fopen(p.string().c_str(), "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END);
	const long n = ftell(f);
	fseek(f, 0, SEEK_SET);
	out->resize(n > 0 ? (size_t)n : 0);
	const size_t got = n > 0 ? fread(out->data(), 1, (size_t)n, f) : 0;
	fclose(f);
	return got == out->size() && n > 0;
}

// the plane of one component, blocks_w * 8 x blocks_h * 8 samples, from its records: block after block
std::vector<uint8_t> reconstruct_plane(const dvpjdmid::Decoder& d, const dvpjdmid::Component& c) {
	const size_t pitch = (size_t)c.blocks_w * 8;
	std::vector<uint8_t> plane(pitch * c.blocks_h * 8);
	for (int by = 0; by < c.blocks_h; ++by)
		for (int bx = 0; bx < c.blocks_w; ++bx) {
			const size_t b = (size_t)by * c.blocks_w + bx;
			dvpjd::reconstruct_block(c.records.data() + c.offsets[b], c.offsets[b + 1] - c.offsets[b], d.qt[c.tq], plane.data() + (size_t)by * 8 * pitch + (size_t)bx * 8, pitch);
		}
	return plane;
}

}  // namespace

// channels = 1: luma plane (libjpeg JCS_GRAYSCALE); 3: BGR
Mat DecodeJpeg(const path& file, int channels) {
	std::vector<uint8_t> bytes;
	if (!read_file(file, &bytes)) return Mat();
	dvpjdmid::Decoder d;
	if (!d.decode(bytes.data(), bytes.size(), channels == 1)) {
		std::cerr << "DecodeJpeg: " << file << ": " << d.error << std::endl;
		return Mat();
	}
	const dvpjdmid::Component& Y = d.comps[0];
	const std::vector<uint8_t> y_plane = reconstruct_plane(d, Y);
	if (channels == 1) {
		Mat g(d.height, d.width, CV_8UC1);
		for (int y = 0; y < d.height; ++y) std::memcpy(g.ptr<uint8_t>(y), y_plane.data() + (size_t)y * Y.blocks_w * 8, (size_t)d.width);
		return g;
	}
	const bool colour = d.comps.size() == 3;
	const dvpjdmid::Component& Cb = d.comps[colour ? 1 : 0];
	const dvpjdmid::Component& Cr = d.comps[colour ? 2 : 0];
	const std::vector<uint8_t> cb_plane = colour ? reconstruct_plane(d, Cb) : std::vector<uint8_t>(), cr_plane = colour ? reconstruct_plane(d, Cr) : std::vector<uint8_t>();
	Mat bgr(d.height, d.width, CV_8UC3);
	// the plane column of every image column, once per component (the same for every row)
	const dvpjdmid::Component* comp[3] = { &Y, &Cb, &Cr };
	const std::vector<uint8_t>* plane[3] = { &y_plane, &cb_plane, &cr_plane };
	std::vector<int> col[3];
	for (int i = 0; i < (colour ? 3 : 1); ++i) {
		col[i].resize(d.width);
		for (int x = 0; x < d.width; ++x) col[i][x] = dvpjd::sample_col(x, comp[i]->h, d.hmax);
	}
	for (int y = 0; y < d.height; ++y) {
		uint8_t* o = bgr.ptr<uint8_t>(y);
		const uint8_t* row[3] = { nullptr, nullptr, nullptr };
		for (int i = 0; i < (colour ? 3 : 1); ++i) row[i] = plane[i]->data() + (size_t)dvpjd::sample_row(y, comp[i]->v, d.vmax) * comp[i]->blocks_w * 8;
		const int* cy = col[0].data();
		if (colour) {
			const int *cb = col[1].data(), *cr = col[2].data();
			for (int x = 0; x < d.width; ++x) dvpjd::ycc_to_bgr(row[0][cy[x]], row[1][cb[x]], row[2][cr[x]], o + 3 * x);
		} else {
			for (int x = 0; x < d.width; ++x) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = row[0][cy[x]];
		}
	}
	return bgr;
}
