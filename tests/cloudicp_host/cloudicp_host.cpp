// TEST INFRASTRUCTURE: csrc/dvp_cloudicp.hpp's serial text as a stand-alone program (no device, no library), for
// tests/test_cloudicp_host.py and as the reference of tests/test_gpu_cloudicp.py.  Clouds are files of packed binary32 x y z.
//   cloudicp_host step <src.bin> <tgt.bin> <params.txt> <nearest.out> <e.out> <sums.out>
//       params.txt: words separated by whitespace, numbers as strtod reads them (hexadecimal floats, nan, inf):
//           increment <16 numbers> | distance <d> | cells 27|125 | search brute|grid          (each at most once; distance is required)
//       prints `count <n>`; nearest.out = int32 per source, e.out = binary32 per source, sums.out = 16 doubles
//   cloudicp_host refine <recon.bin> <truth.bin> <params.txt> <matrix.out>
//       params.txt: transform <16 numbers> | crop <axis> <axis_min> <axis_max> <n> <3 n numbers> | cells 27|125 |
//                   stage <voxel> <distance> <iterations>  (in order, any number)
//       prints one line `log <stage> <step> <n_src> <n> <rmse as a hexadecimal float>` per step; matrix.out = 16 doubles
//   cloudicp_host solve <n> <16 sums> <3 reference coordinates>      prints E's 16 numbers as hexadecimal floats
// Exit status 3: the arguments are refused (message on stderr), 1: a file cannot be read or written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../dvp-mvs_amd/csrc/dvp_cloudicp.hpp"

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
static bool WriteBin(const char* file, const T* v, size_t n) {
	std::ofstream out(file, std::ios::binary);
	out.write((const char*)v, (std::streamsize)(n * sizeof(T)));
	return out.good();
}

struct Params {
	double increment[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 }, transform[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	double distance = NAN;
	int R = 1;
	bool brute = false, grid = false;
	dvpcp::Prep crop;
	std::vector<dvpci::Stage> stages;
};

static bool ReadParams(const char* file, Params* p) {
	std::ifstream in(file);
	if (!in.good()) return false;
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
		if (word == "increment" || word == "transform") {
			for (int k = 0; k < 16; ++k)
				if (!number(word == "increment" ? &p->increment[k] : &p->transform[k])) return false;
		} else if (word == "distance") {
			if (!number(&p->distance)) return false;
		} else if (word == "cells") {
			if (!number(&v) || (v != 27.0 && v != 125.0)) return false;
			p->R = v == 27.0 ? 1 : 2;
		} else if (word == "search") {
			if (!(in >> word)) return false;
			p->brute = word == "brute";
			p->grid = word == "grid";
			if (!p->brute && !p->grid) return false;
		} else if (word == "crop") {
			double n;
			if (!number(&v) || !number(&p->crop.axis_min) || !number(&p->crop.axis_max) || !number(&n) || n < 0 || n > 100000) return false;
			p->crop.crop_axis = (int)v;
			p->crop.polygon.resize((size_t)n * 3);
			for (double& c : p->crop.polygon)
				if (!number(&c)) return false;
		} else if (word == "stage") {
			dvpci::Stage s;
			if (!number(&s.voxel) || !number(&s.max_distance) || !number(&v)) return false;
			s.max_iterations = (int)v;
			p->stages.push_back(s);
		} else return false;
	}
	return true;
}

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "step" && argc == 8) {
		const std::vector<float> src = ReadBin(argv[2]), tgt = ReadBin(argv[3]);
		Params p;
		if (!ReadParams(argv[4], &p)) { fprintf(stderr, "cannot read the parameters %s\n", argv[4]); return 1; }
		const long long ns = (long long)(src.size() / 3), nt = (long long)(tgt.size() / 3);
		std::vector<int> nearest((size_t)ns);
		std::vector<float> e((size_t)ns);
		double sums[16];
		long long count = 0;
		const bool brute = p.brute || (!p.grid && ns * nt <= dvpce::kBruteForcePairs);
		const std::string what = dvpci::serial_icp_step(src.data(), ns, tgt.data(), nt, p.increment, (float)p.distance, p.R, brute, nearest.data(), e.data(), sums, &count);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		printf("count %lld\n", count);
		return WriteBin(argv[5], nearest.data(), nearest.size()) && WriteBin(argv[6], e.data(), e.size()) && WriteBin(argv[7], sums, 16) ? 0 : 1;
	}
	if (cmd == "refine" && argc == 6) {
		const std::vector<float> recon = ReadBin(argv[2]), truth = ReadBin(argv[3]);
		Params p;
		if (!ReadParams(argv[4], &p)) { fprintf(stderr, "cannot read the parameters %s\n", argv[4]); return 1; }
		dvpci::HostBackend be;
		be.xyz[0] = recon.data(); be.xyz[1] = truth.data();
		be.num[0] = (long long)(recon.size() / 3); be.num[1] = (long long)(truth.size() / 3);
		be.prep[0] = be.prep[1] = p.crop;
		be.R = p.R;
		dvpcp::Prep whole = p.crop;
		whole.has_transform = true;
		for (int k = 0; k < 16; ++k) whole.m[k] = p.transform[k];
		std::string what = dvpcp::check_prep(whole);
		std::vector<dvpci::LogRecord> log;
		double M[16];
		for (int k = 0; k < 16; ++k) M[k] = p.transform[k];
		if (what.empty()) what = dvpci::refine(be, p.stages.data(), (int)p.stages.size(), M, &log);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		for (const dvpci::LogRecord& r : log) printf("log %d %d %lld %lld %a\n", r.stage, r.step, r.n_src, r.n, r.rmse);
		return WriteBin(argv[5], M, 16) ? 0 : 1;
	}
	if (cmd == "solve" && argc == 22) {
		double v[19], E[16];
		for (int k = 0; k < 19; ++k) v[k] = strtod(argv[3 + k], nullptr);
		dvpci::solve(v, atoll(argv[2]), v + 16, E);
		for (int k = 0; k < 16; ++k) printf("%a%c", E[k], k % 4 == 3 ? '\n' : ' ');
		return 0;
	}
	fprintf(stderr, "usage: cloudicp_host step|refine|solve ... (see the source)\n");
	return 1;
}
