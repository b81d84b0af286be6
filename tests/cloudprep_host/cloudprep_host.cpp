// TEST INFRASTRUCTURE: csrc/dvp_cloudprep.hpp's serial text and host/prepfiles.cpp as a stand-alone program (no device, no library),
// for tests/test_cloudprep_host.py and as the reference of tests/test_gpu_cloudprep.py.  Clouds are files of packed binary32 x y z.
//   cloudprep_host prepare <cloud.bin> <prep.txt> <xyz.out> <index.out>
//       prep.txt: words separated by whitespace, numbers as strtod reads them (hexadecimal floats, nan, inf):
//           transform <16 numbers> | crop <axis> <axis_min> <axis_max> <n> <3 n numbers> | voxel <s>      (each at most once)
//       prints `counts <finite> <after transform> <inside> <out>`; xyz.out = the prepared float triples, index.out = int64 input indices
//   cloudprep_host transform <file>      the --transform reader: prints the 16 numbers as hexadecimal floats
//   cloudprep_host crop <file>           the --crop reader: prints `<axis> <axis_min> <axis_max> <n>` and the vertices, one per line
// Exit status 3: the description or the cloud is refused, 2: a reader refuses its file (message on stderr).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../dvp-mvs_amd/csrc/dvp_cloudprep.hpp"
#include "../../dvp-mvs_amd/host/evaluate.h"

static std::vector<float> ReadBin(const char* file) {
	std::ifstream in(file, std::ios::binary | std::ios::ate);
	if (!in.good()) { fprintf(stderr, "cannot read %s\n", file); exit(1); }
	const size_t bytes = (size_t)in.tellg();
	std::vector<float> v(bytes / 4);
	in.seekg(0);
	in.read((char*)v.data(), (std::streamsize)(v.size() * 4));
	return v;
}

template <class T>
static bool WriteBin(const char* file, const std::vector<T>& v) {
	std::ofstream out(file, std::ios::binary);
	out.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
	return out.good();
}

static bool ReadPrepText(const char* file, dvpcp::Prep* p) {
	std::ifstream in(file);
	std::string word;
	auto number = [&in](double* v) {
		std::string w;
		if (!(in >> w)) return false;
		char* end = nullptr;
		*v = strtod(w.c_str(), &end);
		return end != w.c_str() && !*end;
	};
	while (in >> word) {
		double v;
		if (word == "transform") {
			p->has_transform = true;
			for (int k = 0; k < 16; ++k)
				if (!number(&p->m[k])) return false;
		} else if (word == "crop") {
			double n;
			if (!number(&v) || !number(&p->axis_min) || !number(&p->axis_max) || !number(&n) || n < 0 || n > 100000) return false;
			p->crop_axis = (int)v;
			p->polygon.resize((size_t)n * 3);
			for (double& c : p->polygon)
				if (!number(&c)) return false;
		} else if (word == "voxel") {
			if (!number(&p->voxel)) return false;
		} else return false;
	}
	return true;
}

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	std::string error;
	if (cmd == "transform" && argc == 3) {
		double m[16];
		if (!ReadTransformFile(argv[2], m, &error)) { fprintf(stderr, "%s\n", error.c_str()); return 2; }
		for (int k = 0; k < 16; ++k) printf("%a%c", m[k], k % 4 == 3 ? '\n' : ' ');
		return 0;
	}
	if (cmd == "crop" && argc == 3) {
		dvpcp::Prep p;
		if (!ReadCropFile(argv[2], &p, &error)) { fprintf(stderr, "%s\n", error.c_str()); return 2; }
		printf("%d %a %a %zu\n", p.crop_axis, p.axis_min, p.axis_max, p.polygon.size() / 3);
		for (size_t k = 0; k < p.polygon.size(); k += 3) printf("%a %a %a\n", p.polygon[k], p.polygon[k + 1], p.polygon[k + 2]);
		return 0;
	}
	if (cmd == "prepare" && argc == 6) {
		const std::vector<float> xyz = ReadBin(argv[2]);
		dvpcp::Prep p;
		if (!ReadPrepText(argv[3], &p)) { fprintf(stderr, "cannot read the description %s\n", argv[3]); return 1; }
		std::vector<float> out;
		std::vector<long long> index;
		long long counts[4];
		const std::string what = dvpcp::serial_prepare(xyz.data(), (long long)(xyz.size() / 3), p, &out, &index, counts);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		printf("counts %lld %lld %lld %lld\n", counts[0], counts[1], counts[2], counts[3]);
		return WriteBin(argv[4], out) && WriteBin(argv[5], index) ? 0 : 1;
	}
	fprintf(stderr, "usage: cloudprep_host prepare|transform|crop ... (see the source)\n");
	return 1;
}
