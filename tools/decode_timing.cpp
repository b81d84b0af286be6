// decode_timing.cpp — where the host JPEG decoder's time goes, on one file, single-threaded (built and run by tools/decode_timing.py).
// The three parts are the ones host/jpeg.cpp's DecodeJpeg runs, from the same headers:
//   (a) marker parse + entropy decode -> coefficient records            csrc/dvp_jpeg_dec_mid.hpp
//   (b) per block: records -> dequantise -> inverse DCT -> clamp -> plane   csrc/dvp_jpeg_dec.hpp
//   (c) three channels only: per pixel chroma sampling + colour equations
// and what `apd --entropy-on gpu` leaves on the host in place of (a): the marker parse up to the scan and the pre-scan that finds
// the segments and lays out the subsequences (csrc/dvp_jpeg_huff.hpp plan()), with the bytes that then go up.
// usage: decode_timing file.jpg repeats      prints one line per channel count, medians in milliseconds
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dvp-mvs_amd/csrc/dvp_jpeg_dec.hpp"
#include "../dvp-mvs_amd/csrc/dvp_jpeg_dec_mid.hpp"
#include "../dvp-mvs_amd/csrc/dvp_jpeg_huff.hpp"

using clock_type = std::chrono::steady_clock;
static double ms(clock_type::time_point a, clock_type::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
	if (argc != 3) { printf("usage: decode_timing file.jpg repeats\n"); return 64; }
	std::vector<uint8_t> file;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 1;
	uint8_t buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + n);
	fclose(f);
	const int repeats = std::max(1, atoi(argv[2]));
	for (int channels : { 1, 3 }) {
		std::vector<double> ta, tb, tc, tp;
		long long upload_bytes = 0, subsequences = 0, segments = 0;
		long long record_bytes = 0, blocks = 0, pixels = 0;
		unsigned checksum = 0;
		for (int r = 0; r < repeats; ++r) {
			{   // the host's share of the device path: parse to the scan + pre-scan
				const clock_type::time_point p0 = clock_type::now();
				dvpjdmid::Decoder h;
				h.stop_at_scan = true;
				dvpjh::Plan plan;
				if (h.decode(file.data(), file.size(), channels == 1) && dvpjh::plan(h, channels == 1, dvpjh::kSubseqBytes, &plan)) {
					upload_bytes = (long long)(plan.data_bytes + plan.segs.size() * sizeof(dvpjh::Seg) + (size_t)plan.lanes * 4 + sizeof(dvpjh::Tables));
					subsequences = plan.lanes;
					segments = (long long)plan.segs.size();
				}
				tp.push_back(ms(p0, clock_type::now()));
			}
			const clock_type::time_point t0 = clock_type::now();
			dvpjdmid::Decoder d;
			if (!d.decode(file.data(), file.size(), channels == 1)) { fprintf(stderr, "%s\n", d.error); return 2; }
			const clock_type::time_point t1 = clock_type::now();
			const int nc = channels == 1 ? 1 : (int)d.comps.size();
			std::vector<uint8_t> planes[3];
			record_bytes = blocks = 0;
			for (int i = 0; i < nc; ++i) {
				const dvpjdmid::Component& c = d.comps[i];
				const size_t pitch = (size_t)c.blocks_w * 8, nb = (size_t)c.blocks_w * c.blocks_h;
				planes[i].resize(pitch * c.blocks_h * 8);
				for (size_t b = 0; b < nb; ++b)
					dvpjd::reconstruct_block(c.records.data() + c.offsets[b], c.offsets[b + 1] - c.offsets[b], d.qt[c.tq], planes[i].data() + (b / c.blocks_w) * 8 * pitch + (b % c.blocks_w) * 8, pitch);
				record_bytes += (long long)(c.offsets.size() + c.records.size()) * 4;
				blocks += (long long)nb;
			}
			std::vector<uint8_t> out((size_t)d.width * d.height * channels);
			if (channels == 1)
				for (int y = 0; y < d.height; ++y) std::copy(planes[0].begin() + (size_t)y * d.comps[0].blocks_w * 8, planes[0].begin() + (size_t)y * d.comps[0].blocks_w * 8 + d.width, out.begin() + (size_t)y * d.width);
			const clock_type::time_point t2 = clock_type::now();
			if (channels == 3 && nc == 3) {   // (the plane column of every image column once, the plane rows once per row: as DecodeJpeg)
				std::vector<int> col[3];
				for (int i = 0; i < 3; ++i) {
					col[i].resize(d.width);
					for (int x = 0; x < d.width; ++x) col[i][x] = dvpjd::sample_col(x, d.comps[i].h, d.hmax);
				}
				for (int y = 0; y < d.height; ++y) {
					const uint8_t* row[3];
					for (int i = 0; i < 3; ++i) row[i] = planes[i].data() + (size_t)dvpjd::sample_row(y, d.comps[i].v, d.vmax) * d.comps[i].blocks_w * 8;
					uint8_t* o = out.data() + (size_t)y * d.width * 3;
					for (int x = 0; x < d.width; ++x) dvpjd::ycc_to_bgr(row[0][col[0][x]], row[1][col[1][x]], row[2][col[2][x]], o + 3 * x);
				}
			}
			const clock_type::time_point t3 = clock_type::now();
			ta.push_back(ms(t0, t1)); tb.push_back(ms(t1, t2)); tc.push_back(ms(t2, t3));
			pixels = (long long)d.width * d.height;
			checksum += out[out.size() / 2];
		}
		printf("channels %d entropy_ms %.1f blocks_ms %.1f colour_ms %.1f record_bytes %lld blocks %lld pixels %lld check %u prescan_ms %.2f upload_bytes %lld subsequences %lld segments %lld\n", channels, median(ta), median(tb),
		       median(tc), record_bytes, blocks, pixels, checksum, median(tp), upload_bytes, subsequences, segments);
	}
	return 0;
}
