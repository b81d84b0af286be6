// Host program around the text `apd --convert-from ... --undistort on` shares between its device and its host path (TEST
// INFRASTRUCTURE): runs dvp-mvs_amd/csrc/dvp_undistort.hpp serially, one pixel after the other, and host/colmap.cpp with the option,
// so that the CPU tests hold them against an independent numpy reading without a GPU.  Arrays travel in files of raw little-endian
// values.
//   undistort_host atan IN OUT     IN: doubles >= 0.  OUT: atan_nonneg of each
//   undistort_host image W H PITCH MODEL NUM_PARAMS IN PARAMS OUT     IN: H rows of PITCH bytes; PARAMS: doubles in COLMAP's order
//                                  (at least NUM_PARAMS).  OUT: H rows of 3 W bytes.  "-" for IN, PARAMS or OUT: a null pointer
//   undistort_host model COLMAP_FOLDER SAVE_FOLDER EXT on|off images|no-images [SCALE_FACTOR]
//                                  the converter on the host; with `images` it needs a device for the JPEG encoder once its checks pass
// Exit status 1 with the message on stderr when the text under test reports an error, 2 for a misuse of this program.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_undistort.hpp"
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
	if (cmd == "atan" && argc == 4) {
		const std::vector<char> in = slurp(argv[2]);
		const double* v = reinterpret_cast<const double*>(in.data());
		std::vector<double> out(in.size() / 8);
		for (size_t i = 0; i < out.size(); ++i) out[i] = dvpund::atan_nonneg(v[i]);
		spill(argv[3], out.data(), out.size() * 8);
		return 0;
	}
	if (cmd == "image" && argc == 10) {
		const int w = atoi(argv[2]), h = atoi(argv[3]), model = atoi(argv[5]), num_params = atoi(argv[6]);
		const long long pitch = atoll(argv[4]);
		const bool no_in = std::string(argv[7]) == "-", no_params = std::string(argv[8]) == "-", no_out = std::string(argv[9]) == "-";
		const std::vector<char> in = no_in ? std::vector<char>() : slurp(argv[7]), params = no_params ? std::vector<char>() : slurp(argv[8]);
		std::vector<uint8_t> out((size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0) * 3 + 1);
		const uint8_t* bgr = no_in ? nullptr : reinterpret_cast<const uint8_t*>(in.data());
		const double* p = no_params ? nullptr : reinterpret_cast<const double*>(params.data());
		const std::string what = dvpund::check_undistort(bgr, w, h, pitch, model, p, num_params, no_out ? nullptr : out.data());
		if (!what.empty()) return report(what);
		if (in.size() != (size_t)pitch * h || params.size() < (size_t)num_params * 8) { std::cerr << "image: the input's size does not fit the arguments\n"; return 2; }
		dvpund::undistort_image_serial(dvpund::make_camera(model, p), bgr, w, h, (size_t)pitch, out.data());
		spill(argv[9], out.data(), out.size() - 1);
		return 0;
	}
	if (cmd == "model" && (argc == 7 || argc == 8)) {
		ConvertOptions o;
		o.colmap_folder = argv[2];
		o.save_folder = argv[3];
		o.model_dir = "model";
		o.model_ext = argv[4];
		o.undistort = std::string(argv[5]) == "on";
		o.images = std::string(argv[6]) == "images";
		if (argc > 7) o.scale_factor = atof(argv[7]);
		o.on_gpu = false;
		std::string error;
		if (!ConvertColmap(o, &error)) return report(error);
		return 0;
	}
	std::cerr << "usage: undistort_host atan|image|model ... (see undistort_host.cpp)\n";
	return 2;
}
