// TEST INFRASTRUCTURE: csrc/dvp_mesh.hpp's serial text as a stand-alone program (no device, no library), for tests/test_mesh_host.py
// and as the reference of tests/test_gpu_mesh.py.
//   mesh_host build <scene.bin> <voxel> <truncation> <min_weight> <out prefix>
//       scene.bin: int32 views, then per view the 112-byte camera record, int32 cols, int32 rows, depth (binary32), mask (bytes),
//       b g r (bytes).  Prints `blocks B vertices V faces F` and writes <prefix>.keys (uint64), .sf (binary32), .w (int32), .colour
//       (uint32 x 4), .vertices (binary32 x 3), .colours (bytes x 3), .faces (int32 x 3).
//   mesh_host cull <scene.bin> <voxel> <truncation> <out file>
//       the device's view cull (view_misses_block over block_sphere and cullable) on the blocks the scene allocates: prints `view N
//       cullable 0|1` per view and writes one byte per (block, view), blocks in key order, views within a block: 1 = the view is skipped
//   mesh_host cull_pairs <scene.bin> <pairs.bin> <out file>
//       the same for hand-made pairs: pairs.bin holds records of int32 view, binary32 voxel, binary32 truncation, int32 bx, by, bz; one
//       byte per record
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

struct Scene {
	std::vector<char> bytes;
	std::vector<std::vector<float>> depths;   // (aligned copies)
	std::vector<dvpmesh::View> views;
};

// 0, or the exit status
static int ReadScene(const char* file, Scene* scene) {
	using namespace dvpmesh;
	std::ifstream in(file, std::ios::binary | std::ios::ate);
	if (!in.good()) { fprintf(stderr, "cannot read %s\n", file); return 1; }
	std::vector<char>& bytes = scene->bytes;
	bytes.resize((size_t)in.tellg());
	in.seekg(0);
	in.read(bytes.data(), (std::streamsize)bytes.size());
	size_t at = 0;
	auto take = [&](size_t n) -> const char* {
		if (at + n > bytes.size()) { fprintf(stderr, "%s is cut short\n", file); exit(1); }
		const char* here = bytes.data() + at;
		at += n;
		return here;
	};
	int32_t count;
	memcpy(&count, take(4), 4);
	scene->depths.reserve((size_t)std::max(count, 0));
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
		scene->depths.emplace_back(L);
		memcpy(scene->depths.back().data(), take(L * 4), L * 4);
		v.depth = scene->depths.back().data();
		v.mask = (const uint8_t*)take(L);
		v.bgr = (const uint8_t*)take(L * 3);
		set_centre(&v);
		v.depth_max = masked_depth_max(v);
		scene->views.push_back(v);
	}
	return 0;
}

static uint8_t Culled(const dvpmesh::View& v, const int at[3], float s, float tau) {
	float C[3], radius;
	dvpmesh::block_sphere(at, s, C, &radius);
	return dvpmesh::view_misses_block(v, dvpmesh::cullable(v.cam), C, radius, tau) ? 1 : 0;
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
	if (cmd == "cull" && argc == 6) {
		Params p;
		const std::string what = check_params(strtof(argv[3], nullptr), strtof(argv[4], nullptr), 1, &p);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		Scene scene;
		const int bad = ReadScene(argv[2], &scene);
		if (bad) return bad;
		std::vector<uint64_t> keys;
		const std::string refused = serial_blocks(scene.views, p, &keys);
		if (!refused.empty()) { fprintf(stderr, "%s\n", refused.c_str()); return 3; }
		for (size_t n = 0; n < scene.views.size(); ++n) printf("view %zu cullable %d\n", n, cullable(scene.views[n].cam) ? 1 : 0);
		std::vector<uint8_t> out;
		for (uint64_t key : keys) {
			int at[3];
			key_block(key, at);
			for (const View& v : scene.views) out.push_back(Culled(v, at, p.s, p.tau));
		}
		return WriteBin(argv[5], out) ? 0 : 1;
	}
	if (cmd == "cull_pairs" && argc == 5) {
		Scene scene;
		const int bad = ReadScene(argv[2], &scene);
		if (bad) return bad;
		std::ifstream in(argv[3], std::ios::binary | std::ios::ate);
		if (!in.good()) { fprintf(stderr, "cannot read %s\n", argv[3]); return 1; }
		struct Pair { int32_t view; float s, tau; int32_t at[3]; };
		std::vector<Pair> pairs((size_t)in.tellg() / sizeof(Pair));
		in.seekg(0);
		in.read((char*)pairs.data(), (std::streamsize)(pairs.size() * sizeof(Pair)));
		std::vector<uint8_t> out;
		for (const Pair& q : pairs) {
			if (q.view < 0 || (size_t)q.view >= scene.views.size()) { fprintf(stderr, "no view %d\n", (int)q.view); return 1; }
			out.push_back(Culled(scene.views[(size_t)q.view], q.at, q.s, q.tau));
		}
		return WriteBin(argv[4], out) ? 0 : 1;
	}
	if (cmd == "build" && argc == 7) {
		Params p;
		const std::string what = check_params(strtof(argv[3], nullptr), strtof(argv[4], nullptr), atoi(argv[5]), &p);
		if (!what.empty()) { fprintf(stderr, "%s\n", what.c_str()); return 3; }
		Scene scene;
		const int bad = ReadScene(argv[2], &scene);
		if (bad) return bad;
		const std::vector<View>& views = scene.views;
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
	fprintf(stderr, "usage: mesh_host build|cull|cull_pairs|vertices|cell|edge ... (see the source)\n");
	return 1;
}
