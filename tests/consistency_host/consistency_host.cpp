// TEST INFRASTRUCTURE: host/fusion.cpp's ConsistencyMaskHost — the serial twin of dvp_fuse_consistency — as a program, for
// tests/test_mesh_consistency_host.py and as the reference of tests/test_gpu_mesh_consistency.py.  No device is used.
//   consistency_host <scene.bin> <ref> <s0,s1,...|-> <min_views> <mask.out>
//       scene.bin: int32 views, then per view the 112-byte camera record, int32 cols, int32 rows, depth (binary32), normals (binary32
//       x 3), int32 has_block, and with it the block mask (bytes).  mask.out: rows * cols bytes of view <ref>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../dvp-mvs_amd/host/APD.h"

int main(int argc, char** argv) {
	if (argc != 6) { fprintf(stderr, "usage: consistency_host scene.bin ref sources min_views mask.out\n"); return 1; }
	std::ifstream in(argv[1], std::ios::binary | std::ios::ate);
	if (!in.good()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
	std::vector<char> bytes((size_t)in.tellg());
	in.seekg(0);
	in.read(bytes.data(), (std::streamsize)bytes.size());
	size_t at = 0;
	auto take = [&](size_t n) -> const char* {
		if (at + n > bytes.size()) { fprintf(stderr, "%s is cut short\n", argv[1]); exit(1); }
		const char* here = bytes.data() + at;
		at += n;
		return here;
	};
	int32_t count;
	memcpy(&count, take(4), 4);
	static_assert(sizeof(Camera) == 112, "the camera record");
	std::vector<ConsistencyView> views((size_t)std::max(count, 0));
	std::vector<std::vector<float>> floats;   // (aligned copies)
	floats.reserve(2 * views.size());
	for (ConsistencyView& v : views) {
		memcpy(&v.cam, take(sizeof(Camera)), sizeof(Camera));
		int32_t size[2];
		memcpy(size, take(8), 8);
		v.cols = size[0];
		v.rows = size[1];
		const size_t L = (size_t)v.cols * v.rows;
		floats.emplace_back(L);
		memcpy(floats.back().data(), take(L * 4), L * 4);
		v.depth = floats.back().data();
		floats.emplace_back(3 * L);
		memcpy(floats.back().data(), take(L * 12), L * 12);
		v.normal = floats.back().data();
		int32_t has_block;
		memcpy(&has_block, take(4), 4);
		v.block = has_block ? (const uint8_t*)take(L) : nullptr;
	}
	const int ref = atoi(argv[2]);
	std::vector<int> src;
	if (std::string(argv[3]) != "-") {
		std::stringstream list(argv[3]);
		std::string item;
		while (std::getline(list, item, ',')) src.push_back(atoi(item.c_str()));
	}
	if (ref < 0 || ref >= count) { fprintf(stderr, "no view %d\n", ref); return 1; }
	for (int s : src)
		if (s < 0 || s >= count) { fprintf(stderr, "no view %d\n", s); return 1; }
	std::vector<uint8_t> mask((size_t)views[ref].cols * views[ref].rows);
	ConsistencyMaskHost(views, ref, src, atoi(argv[4]), mask.data());
	std::ofstream out(argv[5], std::ios::binary);
	out.write((const char*)mask.data(), (std::streamsize)mask.size());
	return out.good() ? 0 : 1;
}
