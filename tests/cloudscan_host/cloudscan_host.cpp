// TEST INFRASTRUCTURE: csrc/dvp_cloudscan.hpp's serial text and host/prepfiles.cpp's MeshLab project reader as a stand-alone program
// (no device, no library), for tests/test_cloudscan_host.py and as the reference of tests/test_gpu_cloudscan.py.  Clouds are files of
// packed binary32 x y z; numbers in text files are read by strtod (hexadecimal floats, nan, inf).
//   scans.txt: one scan per line: <points.bin> <16 numbers> [<count>]     (a count of its own, for the argument checks)
//   prep.txt:  transform <16 numbers> | crop <axis> <axis_min> <axis_max> <n> <3 n numbers> | voxel <s> | none
//   cloudscan_host gaps <scans.txt> <R> <query.bin> <gap.out> <maps.out> <truth.out>
//       gap.out = binary32 per query, maps.out = S * 6 R R binary32, truth.out = the truth cloud
//   cloudscan_host evaluate <recon.bin> <scans.txt> <R> <tolerances.txt> <prep_recon.txt> <prep_truth.txt> <d2.out> <gap.out> <recon.out> <truth.out>
//       prints `within_recon`, `within_truth`, `used`, `free_space`, `counts`, each followed by its integers; d2.out / gap.out per
//       prepared reconstructed point, recon.out / truth.out the prepared clouds
//   cloudscan_host mlp <project.mlp>      prints per scan: <name> <path> and the 16 numbers as hexadecimal floats
// Exit status 3: the arguments are refused (message on stderr), 2: the project is refused, 1: a file cannot be read or written.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "../../dvp-mvs_amd/csrc/dvp_cloudscan.hpp"
#include "../../dvp-mvs_amd/host/evaluate.h"

static std::vector<float> ReadBin(const std::string& file) {
	std::ifstream in(file, std::ios::binary | std::ios::ate);
	if (!in.good()) { fprintf(stderr, "cannot read %s\n", file.c_str()); exit(1); }
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

static bool Number(std::istream& in, double* v) {
	std::string w;
	if (!(in >> w)) return false;
	char* end = nullptr;
	*v = strtod(w.c_str(), &end);
	return end != w.c_str() && !*end;
}

struct Scans {
	std::vector<std::vector<float>> points;
	std::vector<dvpcs::Scan> list;
};

static void ReadScans(const char* file, Scans* scans) {
	std::ifstream in(file);
	if (!in.good()) { fprintf(stderr, "cannot read %s\n", file); exit(1); }
	std::string line;
	while (std::getline(in, line)) {
		std::stringstream words(line);
		std::string bin;
		if (!(words >> bin)) continue;
		scans->points.push_back(ReadBin(bin));
		dvpcs::Scan s;
		for (int k = 0; k < 16; ++k)
			if (!Number(words, &s.m[k])) { fprintf(stderr, "cannot read the scans %s\n", file); exit(1); }
		double count;
		s.num = Number(words, &count) ? (long long)count : (long long)(scans->points.back().size() / 3);
		scans->list.push_back(s);
	}
	for (size_t k = 0; k < scans->list.size(); ++k) scans->list[k].xyz = scans->points[k].data();
}

// false: the file cannot be read; *given = it holds a description
static bool ReadPrep(const char* file, dvpcp::Prep* p, bool* given) {
	std::ifstream in(file);
	if (!in.good()) return false;
	std::string word;
	*given = false;
	while (in >> word) {
		double v, n;
		if (word == "none") return true;
		*given = true;
		if (word == "transform") {
			p->has_transform = true;
			for (int k = 0; k < 16; ++k)
				if (!Number(in, &p->m[k])) return false;
		} else if (word == "crop") {
			if (!Number(in, &v) || !Number(in, &p->axis_min) || !Number(in, &p->axis_max) || !Number(in, &n) || n < 0 || n > 100000) return false;
			p->crop_axis = (int)v;
			p->polygon.resize((size_t)n * 3);
			for (double& c : p->polygon)
				if (!Number(in, &c)) return false;
		} else if (word == "voxel") {
			if (!Number(in, &p->voxel)) return false;
		} else return false;
	}
	return true;
}

static void PrintCounts(const char* name, const long long* v, int n) {
	printf("%s", name);
	for (int k = 0; k < n; ++k) printf(" %lld", v[k]);
	printf("\n");
}

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "gaps" && argc == 8) {
		Scans scans;
		ReadScans(argv[2], &scans);
		const int R = atoi(argv[3]);
		const std::vector<float> query = ReadBin(argv[4]);
		long long total = 0;
		std::string what = dvpcs::check_cube(R);
		if (what.empty()) what = dvpcs::check_scans(scans.list.data(), (int)scans.list.size(), &total);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		std::vector<float> truth, maps, gap(query.size() / 3);
		dvpcs::serial_truth(scans.list.data(), (int)scans.list.size(), &truth);
		dvpcs::serial_maps(scans.list.data(), (int)scans.list.size(), truth.data(), R, &maps);
		dvpcs::serial_gaps(query.data(), (long long)gap.size(), scans.list.data(), (int)scans.list.size(), R, maps.data(), gap.data());
		return WriteBin(argv[5], gap) && WriteBin(argv[6], maps) && WriteBin(argv[7], truth) ? 0 : 1;
	}
	if (cmd == "evaluate" && argc == 12) {
		const std::vector<float> recon = ReadBin(argv[2]);
		Scans scans;
		ReadScans(argv[3], &scans);
		const int R = atoi(argv[4]);
		std::vector<float> tol;
		{
			std::ifstream in(argv[5]);
			double v;
			while (Number(in, &v)) tol.push_back((float)v);
		}
		dvpcp::Prep prep[2];
		bool given[2];
		for (int c = 0; c < 2; ++c)
			if (!ReadPrep(argv[6 + c], &prep[c], &given[c])) { fprintf(stderr, "cannot read the preparation %s\n", argv[6 + c]); return 1; }
		long long within_recon[dvpce::kMaxTolerances] = {}, within_truth[dvpce::kMaxTolerances] = {}, used[2] = {}, free_space[dvpce::kMaxTolerances] = {}, counts[8] = {};
		std::vector<float> prepared[2], d2, gap;
		const std::string what = tol.size() > (size_t)dvpce::kMaxTolerances ? "at most 8 tolerances" : dvpcs::serial_evaluate_scans(recon.data(), (long long)(recon.size() / 3), given[0] ? &prep[0] : nullptr,
			scans.list.data(), (int)scans.list.size(), given[1] ? &prep[1] : nullptr, R, tol.data(), (int)tol.size(), within_recon, within_truth, used, free_space, counts, prepared, &d2, &gap);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		const int K = (int)tol.size();
		PrintCounts("within_recon", within_recon, K);
		PrintCounts("within_truth", within_truth, K);
		PrintCounts("used", used, 2);
		PrintCounts("free_space", free_space, K);
		PrintCounts("counts", counts, 8);
		return WriteBin(argv[8], d2) && WriteBin(argv[9], gap) && WriteBin(argv[10], prepared[0]) && WriteBin(argv[11], prepared[1]) ? 0 : 1;
	}
	if (cmd == "mlp" && argc == 3) {
		std::vector<ScanEntry> entries;
		std::string error;
		if (!ReadScanProject(argv[2], &entries, &error)) { fprintf(stderr, "%s\n", error.c_str()); return 2; }
		for (const ScanEntry& e : entries) {
			printf("%s %s", e.name.c_str(), e.path.c_str());
			for (int k = 0; k < 16; ++k) printf(" %a", e.m[k]);
			printf("\n");
		}
		return 0;
	}
	fprintf(stderr, "usage: cloudscan_host gaps|evaluate|mlp ... (see the source)\n");
	return 1;
}
