// TEST INFRASTRUCTURE: csrc/dvp_mesh.hpp's serial text as a stand-alone program (no device, no library), for tests/test_mesh_host.py
// and as the reference of tests/test_gpu_mesh.py.
//   mesh_host build <scene.bin> <voxel> <truncation> <min_weight> <out prefix>
//       scene.bin: int32 views, then per view the 112-byte camera record, int32 cols, int32 rows, depth (binary32), mask (bytes),
//       b g r (bytes).  Prints `blocks B vertices V faces F` and writes <prefix>.keys (uint64), .sf (binary32), .w (int32), .colour
//       (uint32 x 4), .vertices (binary32 x 3), .colours (bytes x 3), .faces (int32 x 3).
//   mesh_host vertices <count>       the refusal of a mesh with that many vertices, or nothing
//   mesh_host cell <F0> ... <F7>     `inactive`, or `active x y z`: the vertex of the cell (0, 0, 0) at voxel 1 with these corner values
//   mesh_host edge <F0> <F1>         edge_face's answer: 0 no face, 1 F rises, 2 F falls
// Exit status 3: refused (message on stderr).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../../dvp-mvs_amd/csrc/dvp_mesh.hpp"

template <class T>
static bool WriteBin(const std::string& file, const std::vector<T>& v) {
	std::ofstream out(file, std::ios::binary);
	out.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
	return out.good();
}

int main(int argc, char** argv) {
	using namespace dvpmesh;
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "vertices" && argc == 3) {
		const long long n = atoll(argv[2]);
		if (n > kMaxVertices) { fprintf(stderr, "%s\n", vertex_refusal(n).c_str()); return 3; }
		return 0;
	}
	if (cmd == "cell" && argc == 10) {   // a hand-made cell at the lattice origin, voxel 1
		float F[8];
		for (int c = 0; c < 8; ++c) F[c] = strtof(argv[2 + c], nullptr);
		if (!cell_active(F)) { printf("inactive\n"); return 0; }
		float X[3];
		cell_vertex(F, 0, 0, 0, 1.0f, X);
		printf("active %.9g %.9g %.9g\n", (double)X[0], (double)X[1], (double)X[2]);
		return 0;
	}
	if (cmd == "edge" && argc == 4) {
		printf("%d\n", edge_face(strtof(argv[2], nullptr), strtof(argv[3], nullptr)));
		return 0;
	}
	if (cmd == "build" && argc == 7) {
		Params p;
		const std::string what = check_params(strtof(argv[3], nullptr), strtof(argv[4], nullptr), atoi(argv[5]), &p);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
		if (!in.good()) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
		std::vector<char> bytes((size_t)in.tellg());
		in.seekg(0);
		in.read(bytes.data(), (std::streamsize)bytes.size());
		size_t at = 0;
		auto take = [&](size_t n) -> const char* {
			if (at + n > bytes.size()) { fprintf(stderr, "%s is cut short\n", argv[2]); exit(1); }
			const char* here = bytes.data() + at;
			at += n;
			return here;
		};
		int32_t count;
		memcpy(&count, take(4), 4);
		std::vector<View> views;
		std::vector<std::vector<float>> depths;   // (aligned copies)
		depths.reserve((size_t)std::max(count, 0));
		for (int n = 0; n < count; ++n) {
			View v;
			memcpy(&v.cam, take(sizeof(DvpCamera)), sizeof(DvpCamera));
			int32_t size[2];
			memcpy(size, take(8), 8);
			const std::string bad = check_view(size[0], size[1]);
			if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 3; }
			v.cols = size[0];
			v.rows = size[1];
			const size_t L = (size_t)v.cols * v.rows;
			depths.emplace_back(L);
			memcpy(depths.back().data(), take(L * 4), L * 4);
			v.depth = depths.back().data();
			v.mask = (const uint8_t*)take(L);
			v.bgr = (const uint8_t*)take(L * 3);
			set_centre(&v);
			v.depth_max = masked_depth_max(v);
			views.push_back(v);
		}
		Volume vol;
		Mesh mesh;
		const std::string refused = serial_build(views, p, &vol, &mesh);
		if (!refused.empty()) { fprintf(stderr, "%s\n", refused.c_str()); return 3; }
		printf("blocks %zu vertices %zu faces %zu\n", vol.keys.size(), mesh.vertices.size() / 3, mesh.faces.size() / 3);
		const std::string prefix = argv[6];
		const bool ok = WriteBin(prefix + ".keys", vol.keys) && WriteBin(prefix + ".sf", vol.sf) && WriteBin(prefix + ".w", vol.w) && WriteBin(prefix + ".colour", vol.colour) &&
		                WriteBin(prefix + ".vertices", mesh.vertices) && WriteBin(prefix + ".colours", mesh.colours) && WriteBin(prefix + ".faces", mesh.faces);
		return ok ? 0 : 1;
	}
	fprintf(stderr, "usage: mesh_host build|vertices ... (see the source)\n");
	return 1;
}
