// Host program around the text `apd --convert-from` shares between its device and its host path (TEST INFRASTRUCTURE): runs
// dvp-mvs_amd/csrc/dvp_pairs.hpp serially, one item after the other, and host/colmap.cpp's readers, formatter and writers, so that
// the CPU tests hold them against the reference's own files and an independent numpy reading without a GPU.  Arrays travel in
// files of raw little-endian values.
//   convert_host scores IN OUT     IN: int64 N, E, P; int64 offsets[N + 1]; int64 ids[E]; double centres[3 N]; int64 point_ids[P];
//                                  double xyz[3 P].  OUT: uint32 score[N * N]
//   convert_host pairs IN OUT      IN: int64 N; uint32 score[N * N].  OUT: the text of pair.txt
//   convert_host fmt IN OUT        IN: doubles.  OUT: one str(float) per line
//   convert_host nn W H PAD_W PAD_H OUT_W OUT_H IN OUT     IN: H rows of 3 W bytes.  OUT: OUT_H rows of 3 OUT_W bytes
//   convert_host model COLMAP_FOLDER SAVE_FOLDER EXT [SCALE_FACTOR [MAX_D [INTERVAL_SCALE]]]    pair.txt, cams/ and sfm/, no images
// Exit status 1 with the message on stderr when the text under test reports an error, 2 for a misuse of this program.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_pairs.hpp"
#include "../../dvp-mvs_amd/host/colmap.h"

namespace {

std::vector<char> slurp(const char* file) {
	std::ifstream in(file, std::ios::binary);
	if (!in) { std::cerr << "cannot open " << file << "\n"; exit(2); }
	return std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}
void spill(const char* file, const void* data, size_t bytes) {
	std::ofstream out(file, std::ios::binary | std::ios::trunc);
	out.write(static_cast<const char*>(data), (std::streamsize)bytes);
	if (!out) { std::cerr << "cannot write " << file << "\n"; exit(2); }
}
int report(const std::string& what) { std::cerr << what << "\n"; return 1; }

}   // namespace

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "scores" && argc == 4) {
		const std::vector<char> in = slurp(argv[2]);
		const long long* head = reinterpret_cast<const long long*>(in.data());
		if (in.size() < 24) return 2;
		const long long N = head[0], E = head[1], P = head[2];
		if (N < 0 || E < 0 || P < 0 || in.size() != (size_t)(24 + 8 * (N + 1) + 8 * E + 24 * N + 8 * P + 24 * P)) { std::cerr << "scores: the input's size does not fit its header\n"; return 2; }
		const long long* offsets = head + 3;
		const long long* ids = offsets + N + 1;
		const double* centres = reinterpret_cast<const double*>(ids + E);
		const long long* point_ids = reinterpret_cast<const long long*>(centres + 3 * N);
		const double* xyz = reinterpret_cast<const double*>(point_ids + P);
		std::vector<uint32_t> score((size_t)(N > 0 ? N * N : 0));
		const std::string what = dvppairs::view_scores_serial((int)N, offsets, ids, centres, P, point_ids, xyz, score.data());
		if (!what.empty()) return report(what);
		spill(argv[3], score.data(), score.size() * 4);
		return 0;
	}
	if (cmd == "pairs" && argc == 4) {
		const std::vector<char> in = slurp(argv[2]);
		if (in.size() < 8) return 2;
		const long long N = *reinterpret_cast<const long long*>(in.data());
		if (N < 1 || in.size() != (size_t)(8 + 4 * N * N)) return 2;
		const std::string text = PairText(reinterpret_cast<const uint32_t*>(in.data() + 8), (int)N);
		spill(argv[3], text.data(), text.size());
		return 0;
	}
	if (cmd == "fmt" && argc == 4) {
		const std::vector<char> in = slurp(argv[2]);
		const double* v = reinterpret_cast<const double*>(in.data());
		std::string text;
		for (size_t i = 0; i < in.size() / 8; ++i) text += PyFloatStr(v[i]) + "\n";
		spill(argv[3], text.data(), text.size());
		return 0;
	}
	if (cmd == "nn" && argc == 10) {
		const int w = atoi(argv[2]), h = atoi(argv[3]), pad_w = atoi(argv[4]), pad_h = atoi(argv[5]), out_w = atoi(argv[6]), out_h = atoi(argv[7]);
		const std::vector<char> in = slurp(argv[8]);
		std::vector<uint8_t> out((size_t)(out_w > 0 ? out_w : 0) * (size_t)(out_h > 0 ? out_h : 0) * 3 + 1);
		if (w > 0 && h > 0 && in.size() != (size_t)w * h * 3) return 2;
		const std::string what = dvppairs::check_convert(in.data(), w, h, 3ll * w, pad_w, pad_h, out_w, out_h, out.data());
		if (!what.empty()) return report(what);
		dvppairs::convert_image_serial(reinterpret_cast<const uint8_t*>(in.data()), w, h, 3 * (size_t)w, pad_w, pad_h, out_w, out_h, out.data());
		spill(argv[9], out.data(), out.size() - 1);
		return 0;
	}
	if (cmd == "model" && argc >= 5 && argc <= 8) {
		ConvertOptions o;
		o.colmap_folder = argv[2];
		o.save_folder = argv[3];
		o.model_dir = ".";
		o.model_ext = argv[4];
		if (argc > 5) o.scale_factor = atof(argv[5]);
		if (argc > 6) o.max_d = atoi(argv[6]);
		if (argc > 7) o.interval_scale = atof(argv[7]);
		o.on_gpu = false;
		o.images = false;
		std::string error;
		if (!ConvertColmap(o, &error)) return report(error);
		return 0;
	}
	std::cerr << "usage: convert_host scores|pairs|fmt|nn|model ... (see convert_host.cpp)\n";
	return 2;
}
