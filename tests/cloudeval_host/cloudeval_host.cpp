// TEST INFRASTRUCTURE: csrc/dvp_cloudeval.hpp's serial text and host/ply.cpp as a stand-alone program (no device, no library), for
// tests/test_evaluate_host.py and as the reference of tests/test_gpu_evaluate.py.  Clouds are files of packed binary32 x y z.
//   cloudeval_host evaluate <recon.bin> <truth.bin> <t0,t1,...> brute|grid <d2.out>
//       prints `used R T`, `within_recon ...`, `within_truth ...`; d2.out = d2 of every recon point, then of every truth point
//   cloudeval_host distances <query.bin> <target.bin> <T> brute|grid <d2.out>      one direction only: d2 of every query
//   cloudeval_host slot <recon.bin> <truth.bin> <T> <x> <y> <z>
//       prints `<capacity> <home slot> <key>` of the cell of (x, y, z) in the grid and table of the two clouds
//   cloudeval_host binned <count>                      make_grid's answer to that many finite points: the table's capacity, or the refusal
//   cloudeval_host ply <file.ply> <xyz.out>            the reader; exit status 2 and the message on stderr when it refuses
// Exit status 3: the clouds or tolerances are refused (message on stderr).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../dvp-mvs_amd/csrc/dvp_cloudeval.hpp"
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

static bool WriteBin(const char* file, const std::vector<float>& v) {
	std::ofstream out(file, std::ios::binary);
	out.write((const char*)v.data(), (std::streamsize)(v.size() * 4));
	return out.good();
}

int main(int argc, char** argv) {
	using namespace dvpce;
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "ply" && argc == 4) {
		std::vector<float> xyz;
		std::string error;
		if (!ReadPlyVertices(argv[2], &xyz, &error)) { fprintf(stderr, "%s\n", error.c_str()); return 2; }
		printf("%zu\n", xyz.size() / 3);
		return WriteBin(argv[3], xyz) ? 0 : 1;
	}
	if (cmd == "binned" && argc == 3) {
		Bounds b;
		b.finite = atoll(argv[2]);
		Grid g;
		const std::string what = make_grid(b, 1.0f, &g);   // (no bounds yet: the count is all that can be wrong)
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		printf("%llu\n", (unsigned long long)table_capacity((uint64_t)b.finite));
		return 0;
	}
	if (((cmd == "evaluate" || cmd == "distances") && argc == 7) || (cmd == "slot" && argc == 8)) {
		const std::vector<float> recon = ReadBin(argv[2]), truth = ReadBin(argv[3]);
		const long long nr = (long long)(recon.size() / 3), nt = (long long)(truth.size() / 3);
		std::vector<float> tol;
		std::stringstream list(argv[4]);
		std::string item;
		while (std::getline(list, item, ',')) tol.push_back(strtof(item.c_str(), nullptr));
		const std::string what = check_tolerances(tol.data(), (int)tol.size());
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		const float T = tol.back();
		Bounds b;
		b.add(recon.data(), nr);
		const long long finite_recon = b.finite;
		b.add(truth.data(), nt);
		Grid g;
		const std::string extent = make_grid(b, T, &g);
		if (!extent.empty()) { fprintf(stderr, "%s\n", extent.c_str()); return 3; }
		if (cmd == "slot") {
			const uint64_t cap = table_capacity((uint64_t)b.finite), key = cell_key(g, strtof(argv[5], nullptr), strtof(argv[6], nullptr), strtof(argv[7], nullptr));
			printf("%llu %llu %llu\n", (unsigned long long)cap, (unsigned long long)(hash_key(key) & (cap - 1)), (unsigned long long)key);
			return 0;
		}
		const std::string mode = argv[5];
		if (mode != "brute" && mode != "grid") { fprintf(stderr, "brute or grid\n"); return 1; }
		std::vector<float> d2((size_t)(nr + nt));
		serial_distances(g, recon.data(), nr, truth.data(), nt, T, mode == "brute", d2.data());
		if (cmd == "distances") {
			d2.resize((size_t)nr);
			return WriteBin(argv[6], d2) ? 0 : 1;
		}
		serial_distances(g, truth.data(), nt, recon.data(), nr, T, mode == "brute", d2.data() + nr);
		long long within[2][kMaxTolerances], used[2];
		count_within(d2.data(), nr, tol.data(), (int)tol.size(), within[0], &used[0]);
		count_within(d2.data() + nr, nt, tol.data(), (int)tol.size(), within[1], &used[1]);
		printf("used %lld %lld\n", used[0], used[1]);
		for (int c = 0; c < 2; ++c) {
			printf(c == 0 ? "within_recon" : "within_truth");
			for (size_t k = 0; k < tol.size(); ++k) printf(" %lld", within[c][k]);
			printf("\n");
		}
		return WriteBin(argv[6], d2) ? 0 : 1;
	}
	fprintf(stderr, "usage: cloudeval_host evaluate|slot|ply ... (see the source)\n");
	return 1;
}
