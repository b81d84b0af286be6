// host-layer checks that need no GPU: on-disk formats, camera parser, connected components,
// rescale helpers.  Exit code 0 = all passed.
#include <thread>
#include <chrono>
#include "../../dvp-mvs_amd/host/driver.h"
#include "../../dvp-mvs_amd/csrc/dvp_fuse_math.hpp"
#include <cassert>
#include <cmath>
#include <cstdio>
#include <omp.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); return 1; } } while (0)


// ---- model of the reference's visibility-mask regions (APD.cpp:138-346), test infrastructure ---------
// The reference labels the zero pixels in two steps.  Connect: a raster scan that gives a pixel its upper
// neighbour's label (else its left one's, else a new one) and, where both neighbours carry different
// labels, records parent[larger] = smaller — OVERWRITING whatever parent the larger label had, so some
// unions are lost.  Label_Update: every horizontally / vertically adjacent pair of different labels whose
// upper-left pixel lies in [0, rows-1) x [0, cols-1) is merged (its list-of-lists bookkeeping builds
// exactly the equivalence classes of those pairs).  Adjacencies inside the last row (right neighbour) and
// the last column (lower neighbour) are never looked at.  region_size_model returns, per pixel, the size
// of its region under that procedure (0 for 255-pixels).
static std::vector<int> region_size_model(const Mat& img) {
	const int R = img.rows, C = img.cols;
	std::vector<int> lab((size_t)R * C, 0), parent(1, 0);
	auto zero = [&](int y, int x) { return img.at<uint8_t>(y, x) == 0; };
	for (int y = 0; y < R; ++y)
		for (int x = 0; x < C; ++x) {
			if (img.at<uint8_t>(y, x) == 255) continue;
			const bool l = x > 0 && zero(y, x) && zero(y, x - 1), u = y > 0 && zero(y, x) && zero(y - 1, x);
			int v = 0;
			if (l) v = lab[(size_t)y * C + x - 1];
			if (u) v = lab[(size_t)(y - 1) * C + x];
			if (!l && !u) { v = (int)parent.size(); parent.push_back(v); }
			if (l && u) {
				const int a = lab[(size_t)y * C + x - 1], b = lab[(size_t)(y - 1) * C + x];
				if (a > b) { parent[a] = b; v = b; }
				else if (a < b) { parent[b] = a; v = a; }
			}
			lab[(size_t)y * C + x] = v;
		}
	std::vector<int> root(parent.size(), 0);
	for (size_t i = 1; i < parent.size(); ++i) { int c = (int)i; while (parent[c] != c) c = parent[c]; root[i] = c; }
	for (auto& v : lab) v = root[v];
	// Label_Update's merges as a union-find over the provisional labels
	std::vector<int> uf(parent.size());
	for (size_t i = 0; i < uf.size(); ++i) uf[i] = (int)i;
	auto find = [&](int a) { while (uf[a] != a) { uf[a] = uf[uf[a]]; a = uf[a]; } return a; };
	for (int y = 0; y + 1 < R; ++y)
		for (int x = 0; x + 1 < C; ++x) {
			const int c = lab[(size_t)y * C + x], r = lab[(size_t)y * C + x + 1], d = lab[(size_t)(y + 1) * C + x];
			if (c != 0 && r != 0 && c != r) uf[find(c)] = find(r);
			if (c != 0 && d != 0 && c != d) uf[find(c)] = find(d);
		}
	std::vector<int> size(parent.size(), 0);
	for (auto v : lab) if (v) size[find(v)]++;
	std::vector<int> out((size_t)R * C, 0);
	for (size_t i = 0; i < lab.size(); ++i) out[i] = lab[i] ? size[find(lab[i])] : 0;
	return out;
}
static std::vector<int> region_size_product(const Mat& img) {   // host/cc.cpp through the reference's two calls
	Mat lab(img.rows, img.cols, CV_32S);
	std::vector<int> cnt;
	Connect(img, lab, cnt);
	Label_Update(lab, cnt);
	std::vector<int> out((size_t)img.rows * img.cols, 0);
	for (int y = 0; y < img.rows; ++y)
		for (int x = 0; x < img.cols; ++x) out[(size_t)y * img.cols + x] = lab.at<int>(y, x) ? cnt[lab.at<int>(y, x)] : 0;
	return out;
}

// `test_host --fuse <dense_folder>`: RunFusion on a folder whose APD/<id>/ maps were written by the caller
// (tests/test_boundary.py::test_fusion_cpu); prints the number of fused points
static int fuse_folder(const path& folder) {
	std::ifstream in(folder / "pair.txt");
	int n = 0;
	in >> n;
	std::vector<Problem> problems;
	for (int i = 0; i < n; ++i) {
		Problem p;
		int k = 0;
		in >> p.ref_image_id >> k;
		p.index = i;
		p.dense_folder = folder;
		p.result_folder = folder / "APD" / ToFormatIndex(p.ref_image_id);
		for (int j = 0; j < k; ++j) { int id; float sc; in >> id >> sc; if (sc > 0) p.src_image_ids.push_back(id); }
		problems.push_back(p);
	}
	const char* on = std::getenv("DVP_FUSION_ON");   // host: the scan on the host's cores; default: the device path (dvp_fuse_*)
	SetFusionOnHost(on && std::string(on) == "host");
	const char* kind = std::getenv("DVP_FUSION_KIND");
	if (kind && std::string(kind) == "tat-intermediate") RunFusion_TAT_Intermediate(folder, problems);
	else if (kind && std::string(kind) == "tat-advanced") RunFusion_TAT_advanced(folder, problems);
	else RunFusion(folder, problems);
	return 0;
}

// `test_host --acos`: the engine's own dvp::fuse_acosf (csrc/dvp_fuse_math.hpp, compiled here as the host library compiles it)
// at every binary32 value in [-1, 1] against acos in double; prints the largest error in units of the last place of the true
// value's binary32 binade, and checks fuse_angle's "rounded past 1 -> 0" and the NaN outside [-1, 1].  Exit 0 = checks passed.
static int acos_contract() {
	const uint32_t top = 0x3f800000u;   // bits of 1.0f: [0, top] are the values 0 .. 1, the same with the sign bit set 0 .. -1
	const int threads = std::max(1, std::min(16, omp_get_num_procs()));
	double worst = 0.0;
	float worst_x = 0.0f;
	long long nan_inside = 0;
#pragma omp parallel num_threads(threads)
	{
		double w = 0.0;
		float wx = 0.0f;
		long long bad = 0;
#pragma omp for schedule(static)
		for (long long i = 0; i <= 2ll * top + 1; ++i) {
			const uint32_t b = i <= top ? (uint32_t)i : 0x80000000u | (uint32_t)(i - top - 1);
			const float x = __builtin_bit_cast(float, b);
			const float r = dvp::fuse_acosf(x);
			const double t = std::acos((double)x);
			if (r != r) { ++bad; continue; }
			int e;
			std::frexp(t, &e);                                  // t in [2^(e-1), 2^e): binary32 ulp there is 2^(e-24)
			const double err = std::fabs((double)r - t) / std::ldexp(1.0, e - 24);
			if (err > w) { w = err; wx = x; }
		}
#pragma omp critical
		{
			if (w > worst) { worst = w; worst_x = wx; }
			nan_inside += bad;
		}
	}
	printf("acos max_ulp %.6f at %.9g (%d threads)\n", worst, worst_x, threads);
	CHECK(nan_inside == 0);
	// NaN outside [-1, 1] and for NaN
	for (float x : { std::nextafter(1.0f, 2.0f), std::nextafter(-1.0f, -2.0f), 2.0f, -3.5f, INFINITY, -INFINITY, NAN }) {
		const float r = dvp::fuse_acosf(x);
		CHECK(r != r);
	}
	CHECK(dvp::fuse_acosf(1.0f) == 0.0f);
	// GetAngle (APD.cpp:1797-1806): a dot product of unit normals that rounds past 1 gives acos = NaN, the angle is 0
	int past_one = 0;
	for (int k = 0; k < 100000; ++k) {
		float v[3] = { std::sin(0.001f * k), std::cos(0.0013f * k), 0.3f + 0.0001f * k };
		const float n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
		for (float& c : v) c /= n;
		const float dot = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
		if (dot > 1.0f) {
			++past_one;
			CHECK(dvp::fuse_angle(v, v) == 0.0f);
		} else {
			CHECK(dvp::fuse_angle(v, v) == dvp::fuse_acosf(dot));
		}
	}
	printf("acos dot_past_one %d\n", past_one);
	CHECK(past_one > 0);
	return 0;
}

// `test_host --jpeg in.jpg out.bin channels`: DecodeJpeg -> raw bytes preceded by int32 rows, cols, channels
static int dump_jpeg(const path& in, const path& out, int channels) {
	const Mat m = DecodeJpeg(in, channels);
	if (m.empty()) return 2;
	std::ofstream f(out, std::ios::binary);
	const int32_t hdr[3] = { m.rows, m.cols, channels };
	f.write((const char*)hdr, 12);
	f.write((const char*)m.data, (std::streamsize)(m.step * m.rows));
	return 0;
}
// `test_host --labels image.pgm scale out.dmb`: LabelSegment -> BinMat (CV_32SC1)
static int dump_labels(const path& in, int scale, const path& out) {
	const Mat img = ReadImageGray(in);
	if (img.empty()) return 2;
	return WriteBinMat(out, EdgeSegment(scale, img, 1)) ? 0 : 3;
}

// `test_host --label-stages image.pgm scale prefix`: LabelSegment with its intermediate maps as BinMat files
// prefix_{quarter,texture,lines,resized,cleaned,labels}.dmb + prefix_n.txt (weak_tex_num)
static int dump_label_stages(const path& in, int scale, const std::string& prefix) {
	const Mat img = ReadImageGray(in);
	if (img.empty()) return 2;
	LabelStages st;
	const Mat lab = LabelSegment(scale, img, &st);
	bool ok = WriteBinMat(prefix + "_quarter.dmb", st.quarter) && WriteBinMat(prefix + "_texture.dmb", st.texture) && WriteBinMat(prefix + "_lines.dmb", st.texture_lines) &&
	          WriteBinMat(prefix + "_resized.dmb", st.resized) && WriteBinMat(prefix + "_cleaned.dmb", st.cleaned) && WriteBinMat(prefix + "_labels.dmb", lab);
	std::ofstream(prefix + "_n.txt") << st.weak_tex_num << "\n";
	return ok ? 0 : 3;
}

// `test_host --edges image.pgm scale out.dmb`: EdgeSegment(scale, image, mode 0, Canny) -> BinMat (CV_8UC1)
static int dump_edges(const path& in, int scale, const path& out) {
	const Mat img = ReadImageGray(in);
	if (img.empty()) return 2;
	return WriteBinMat(out, EdgeSegment(scale, img, 0, true)) ? 0 : 3;
}
// `test_host --prior dense_folder image_id W H out.bin`: BuildPlanePrior (dep/ + sfm/ + cams/) -> W*H float4 (world normal, metric depth)
static int dump_prior(const path& folder, int id, int W, int H, const path& out) {
	Problem p;
	p.ref_image_id = id;
	p.dense_folder = folder;
	p.result_folder = folder / "APD" / ToFormatIndex(id);
	Camera cam;
	if (!ReadCamera(folder / "cams" / (ToFormatIndex(id) + "_cam.txt"), cam)) return 2;
	cam.width = W;
	cam.height = H;
	std::vector<float4> planes((size_t)W * H, float4{ 0, 0, 0, 0 });
	if (!BuildPlanePrior(p, cam, W, H, planes.data())) return 3;
	std::ofstream f(out, std::ios::binary);
	f.write((const char*)planes.data(), (std::streamsize)(planes.size() * sizeof(float4)));
	return f.good() ? 0 : 4;
}

// `test_host --cleanup in.bin W H nsrc min_region out.bin`: CleanSelectedViewsOnHost (what `apd --cleanup-on host` runs) on a raw
// W x H map of 32-bit selected-view words (tests/test_driver_host.py)
static int clean_views(const char* in, int W, int H, int nsrc, int min_region, const char* out) {
	Mat views(H, W, CV_32S);
	std::ifstream f(in, std::ios::binary);
	if (W < 1 || H < 1 || !f.read((char*)views.data, (std::streamsize)views.total() * 4)) return 2;
	CleanSelectedViewsOnHost(views, nsrc, min_region);
	std::ofstream o(out, std::ios::binary);
	o.write((const char*)views.data, (std::streamsize)views.total() * 4);
	return o.good() ? 0 : 3;
}

// `test_host --options <argv...>`: what ParseOptions makes of `apd <argv...>`, one field per line
static int dump_options(int argc, char** argv) {
	const Options o = ParseOptions(argc, argv);
	const RunConfig& r = o.run;
	std::cout << "dense_folder " << o.dense_folder.string() << "\ngpu " << o.gpu << "\nmax_src " << o.max_src << "\niters " << o.iters << "\nmin_scale " << o.min_scale
	          << "\ngeom_passes " << o.geom_passes << "\nrank " << o.rank << "\nworld " << o.world << "\nseed " << o.seed << "\nfusion " << o.fusion << "\njacobi " << o.jacobi
	          << "\ncollective_timeout_s " << o.collective_timeout_s << "\nsync_io " << o.sync_io << "\nhost_rescale " << o.host_rescale << "\npreviews " << o.previews
	          << "\nviews_in_flight " << o.views_in_flight << "\nin_flight_pixels " << o.in_flight_pixels << "\njob " << o.job << "\ntransport " << o.transport
	          << "\nfusion_on_host " << o.fusion_on_host << "\nfusion_kind " << o.fusion_kind << "\nuse_label_files " << r.use_label_files << "\nedges_on_device " << r.edges_on_device
	          << "\ncleanup_on_device " << r.cleanup_on_device << "\nlabels_on_device " << r.labels_on_device << "\nprior_on_device " << r.prior_on_device
	          << "\nimages_on_device " << r.images_on_device << "\ndecode_on_device " << r.decode_on_device << "\ndevice_rescale " << r.device_rescale << "\ndevice_maps " << r.device_maps
	          << "\nstrong_wide " << r.strong_wide << "\nfinal_iteration " << r.final_iteration << "\n";
	return 0;
}

// `test_host --plan round_num min_scale passes`: the pass list, one line per pass — "level scale geom_index" and what ConfigurePass
// leaves in the Problem that is carried from pass to pass, as the driver's are (with --iters 3)
static int dump_plan(int round_num, int min_scale, int passes) {
	const std::vector<Pass> plan = BuildPlan(round_num, min_scale, passes);
	Problem p;
	for (size_t it = 0; it < plan.size(); ++it) {
		ConfigurePass(p, plan[it], (int)it, 3, round_num);
		const PatchMatchParams& q = p.params;
		printf("%d %d %d | iteration %d scale_size %d max_iterations %d state %d use_APD %d use_detail %d geom_consistency %d weak_peak_radius %d rotate_time %d ransac_threshold %.5f\n",
		       plan[it].level, plan[it].scale, plan[it].geom_index, p.iteration, p.scale_size, q.max_iterations, (int)q.state, (int)q.use_APD, (int)q.use_detail, (int)q.geom_consistency,
		       q.weak_peak_radius, q.rotate_time, q.ransac_threshold);
	}
	return 0;
}

int main(int argc, char** argv) {
	if (argc > 7 && std::string(argv[1]) == "--cleanup") return clean_views(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), argv[7]);
	if (argc > 2 && std::string(argv[1]) == "--options") return dump_options(argc - 1, argv + 1);
	if (argc > 4 && std::string(argv[1]) == "--plan") return dump_plan(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
	if (argc > 2 && std::string(argv[1]) == "--fuse") return fuse_folder(argv[2]);
	if (argc > 1 && std::string(argv[1]) == "--acos") return acos_contract();
	if (argc > 6 && std::string(argv[1]) == "--depth-cloud") {   // --depth-cloud depths.dmb image cam out.ply dmin dmax
		Mat depth;
		if (!ReadBinMat(argv[2], depth)) return 2;
		ExportDepthImagePointCloud(argv[5], argv[3], argv[4], depth, (float)atof(argv[6]), argc > 7 ? (float)atof(argv[7]) : 1e30f);
		return 0;
	}
	if (argc > 4 && std::string(argv[1]) == "--edges") return dump_edges(argv[2], std::atoi(argv[3]), argv[4]);
	if (argc > 6 && std::string(argv[1]) == "--prior") return dump_prior(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), argv[6]);
	if (argc > 4 && std::string(argv[1]) == "--jpeg") return dump_jpeg(argv[2], argv[3], std::atoi(argv[4]));
	if (argc > 2 && std::string(argv[1]) == "--image-size") {   // ImageFileSize: "<w> <h>" from the header alone
		int w = 0, h = 0;
		if (!ImageFileSize(argv[2], &w, &h)) return 2;
		printf("%d %d\n", w, h);
		return 0;
	}
	if (argc > 5 && std::string(argv[1]) == "--resize") {   // --resize in.dmb new_cols new_rows out.dmb: ResizeLinear of a float image
		Mat src;
		if (!ReadBinMat(argv[2], src) || src.type() != CV_32FC1) return 2;
		return WriteBinMat(argv[5], ResizeLinear(src, std::atoi(argv[3]), std::atoi(argv[4]))) ? 0 : 3;
	}
	if (argc > 4 && std::string(argv[1]) == "--labels") return dump_labels(argv[2], std::atoi(argv[3]), argv[4]);
	if (argc > 4 && std::string(argv[1]) == "--label-stages") return dump_label_stages(argv[2], std::atoi(argv[3]), argv[4]);
	path tmp = argc > 1 ? path(argv[1]) : std::filesystem::temp_directory_path();
	// BinMat round trips (APD.cpp:548-573, 630-649): header = version 1, rows, cols, cv type
	{
		Mat d(3, 5, CV_32FC1);
		for (int r = 0; r < 3; ++r) for (int c = 0; c < 5; ++c) d.at<float>(r, c) = r * 10 + c + 0.5f;
		CHECK(WriteBinMat(tmp / "t_depth.dmb", d));
		Mat e;
		CHECK(ReadBinMat(tmp / "t_depth.dmb", e));
		CHECK(e.rows == 3 && e.cols == 5 && e.type() == CV_32FC1);
		CHECK(std::memcmp(d.data, e.data, 3 * 5 * 4) == 0);
		FILE* f = fopen((tmp / "t_depth.dmb").string().c_str(), "rb");
		int32_t h[4];
		CHECK(fread(h, 4, 4, f) == 4);
		fclose(f);
		CHECK(h[0] == 1 && h[1] == 3 && h[2] == 5 && h[3] == 5);
		CHECK(std::filesystem::file_size(tmp / "t_depth.dmb") == 16 + 3 * 5 * 4);
		Mat n(2, 2, CV_32FC3), w(2, 2, CV_8UC1), s(2, 2, CV_32SC1);
		CHECK(n.step == 24 && w.step == 2 && s.step == 8 && n.type() == 21 && s.type() == 4);
		CHECK(!ReadBinMat(tmp / "does_not_exist.dmb", e));
		CHECK(writeDepthDmb(tmp / "t_acmm.dmb", d) == 0);
		CHECK(std::filesystem::file_size(tmp / "t_acmm.dmb") == 16 + 3 * 5 * 4);
	}
	// write-back result cache + background worker (host/store.cpp): a published map is served from memory while its file is
	// still being written, a map the reader will modify is never shared with the writer, an announced path makes the reader
	// wait for its job, the files end up on disk byte-identical, eviction keeps working under a tiny limit
	{
		const path dir = tmp / "store_test";
		std::filesystem::create_directories(dir);
		SetResultCache(true, (size_t)1 << 20);
		Mat a(64, 64, CV_32FC1);
		for (int i = 0; i < 64 * 64; ++i) a.ptr<float>(0)[i] = (float)i;
		PublishResult(dir / "a.dmb", a);
		Mat b;
		CHECK(LoadResult(dir / "a.dmb", b));                       // from memory (the write may still be queued)
		CHECK(b.data == a.data || std::memcmp(b.data, a.data, 64 * 64 * 4) == 0);
		Mat c;
		CHECK(LoadResult(dir / "a.dmb", c, true));                 // will_modify: own buffer unless the write is done
		c.ptr<float>(0)[0] = -1.0f;
		FlushResults();
		Mat d;
		CHECK(ReadBinMat(dir / "a.dmb", d) && d.ptr<float>(0)[0] == 0.0f && d.ptr<float>(0)[4095] == 4095.0f);   // the file never saw the modification
		CHECK(!std::filesystem::exists(dir / "a.dmb.part"));
		// announced result: the loader blocks until the background job publishes it
		ExpectResult(dir / "late.dmb");
		RunInBackground([dir]() {
			std::this_thread::sleep_for(std::chrono::milliseconds(150));
			Mat m = Mat::zeros(8, 8, CV_8UC1);
			m.data[5] = 77;
			PublishResult(dir / "late.dmb", m);
		});
		const auto t0 = std::chrono::steady_clock::now();
		Mat late;
		CHECK(LoadResult(dir / "late.dmb", late) && late.data[5] == 77);
		CHECK(std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100));
		CHECK(ResultExists(dir / "late.dmb") && !ResultExists(dir / "never.dmb"));
		// eviction under a 1 MiB limit: 40 maps of 64 KiB; everything is still loadable (memory or file) and intact
		for (int k = 0; k < 40; ++k) {
			Mat m(128, 128, CV_32SC1);
			for (int i = 0; i < 128 * 128; ++i) m.ptr<int>(0)[i] = k * 100000 + i;
			PublishResult(dir / ("m" + std::to_string(k) + ".dmb"), m);
		}
		FlushResults();
		for (int k = 0; k < 40; ++k) {
			Mat m;
			CHECK(LoadResult(dir / ("m" + std::to_string(k) + ".dmb"), m) && m.ptr<int>(0)[777] == k * 100000 + 777);
		}
		// a newer version of a path replaces the older one, in memory and on disk
		Mat v1 = Mat::zeros(4, 4, CV_8UC1), v2 = Mat::zeros(4, 4, CV_8UC1);
		v1.data[0] = 1; v2.data[0] = 2;
		PublishResult(dir / "v.dmb", v1);
		PublishResult(dir / "v.dmb", v2);
		Mat v;
		CHECK(LoadResult(dir / "v.dmb", v) && v.data[0] == 2);
		FlushResults(true);
		CHECK(ReadBinMat(dir / "v.dmb", v) && v.data[0] == 2);
		ShutdownResultStore();
		SetResultCache(true, (size_t)32 << 30);
		std::filesystem::remove_all(dir);
	}
	// camera text (APD.cpp:651-692): c = -R^T t, depth_min interval depth_num depth_max
	{
		std::ofstream f(tmp / "t_cam.txt");
		f << "extrinsic\n0 -1 0 1\n1 0 0 2\n0 0 1 3\n0 0 0 1\n\nintrinsic\n500 0 320\n0 510 240\n0 0 1\n\n2.5 0.02 192 6.5\n";
		f.close();
		Camera cam;
		CHECK(ReadCamera(tmp / "t_cam.txt", cam));
		CHECK(cam.R[1] == -1 && cam.R[3] == 1 && cam.t[2] == 3 && cam.K[0] == 500 && cam.K[4] == 510 && cam.K[5] == 240);
		CHECK(cam.depth_min == 2.5f && cam.depth_max == 6.5f);
		// c_j = -(R[0+j] t0 + R[3+j] t1 + R[6+j] t2)
		CHECK(cam.c[0] == -2.0f && cam.c[1] == 1.0f && cam.c[2] == -3.0f);
		CHECK(!ReadCamera(tmp / "missing_cam.txt", cam));
	}
	CHECK(ToFormatIndex(42) == "00000042");
	// connected components of zero pixels, label 0 = 255-pixels (APD.cpp:233-346)
	{
		const char* rows[5] = { "0.0..", "0.0.0", "...00", "0....", "00.0." };   // '0' = zero pixel, '.' = 255
		Mat m(5, 5, CV_8UC1), lab(5, 5, CV_32S);
		for (int r = 0; r < 5; ++r) for (int c = 0; c < 5; ++c) m.at<uint8_t>(r, c) = rows[r][c] == '0' ? 0 : 255;
		std::vector<int> cnt;
		Connect(m, lab, cnt);
		Label_Update(lab, cnt);
		CHECK(cnt.size() == 6);   // background + 5 components: {0,0;1,0} {0,2;1,2} {1,4;2,3;2,4} {3,0;4,0;4,1} {4,3}
		CHECK(lab.at<int>(0, 0) == lab.at<int>(1, 0) && lab.at<int>(0, 0) != lab.at<int>(0, 2));
		CHECK(lab.at<int>(1, 4) == lab.at<int>(2, 3) && lab.at<int>(2, 3) == lab.at<int>(2, 4));
		CHECK(lab.at<int>(3, 0) == lab.at<int>(4, 1));
		CHECK(cnt[lab.at<int>(1, 4)] == 3 && cnt[lab.at<int>(4, 3)] == 1 && lab.at<int>(0, 1) == 0);
		int total = 0;
		for (int v : cnt) total += v;
		CHECK(total == 25);
	}
	// Visibility-mask regions: exact components (host/cc.cpp) against the model of the reference's
	// Connect + Label_Update on random masks.  (i) a region that touches neither the last row nor the last
	// column has the same size in both; (ii) elsewhere the exact component can only be LARGER (the
	// reference misses merges along the last row / column), so a region the reference keeps (>= threshold)
	// is kept here too.  Reported: how many pixels differ at all.
	{
		uint32_t lcg = 777u;
		auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) * (1.0f / 16777216.0f); };
		long long px_total = 0, px_diff = 0, masks_diff = 0;
		for (int trial = 0; trial < 300; ++trial) {
			const int R = 6 + (int)(rnd() * 40), C = 6 + (int)(rnd() * 40);
			const float density = 0.25f + 0.6f * rnd();
			Mat m(R, C, CV_8UC1);
			for (int y = 0; y < R; ++y) for (int x = 0; x < C; ++x) m.at<uint8_t>(y, x) = rnd() < density ? 0 : 255;
			const std::vector<int> a = region_size_model(m), b = region_size_product(m);
			// pixels of exact components that touch the last row / column
			Mat lab(R, C, CV_32S);
			std::vector<int> cnt;
			Connect(m, lab, cnt);
			std::vector<char> touches(cnt.size(), 0);
			for (int y = 0; y < R; ++y) touches[lab.at<int>(y, C - 1)] = 1;
			for (int x = 0; x < C; ++x) touches[lab.at<int>(R - 1, x)] = 1;
			bool any = false;
			for (int y = 0; y < R; ++y)
				for (int x = 0; x < C; ++x) {
					const size_t i = (size_t)y * C + x;
					px_total++;
					CHECK((a[i] == 0) == (b[i] == 0));
					CHECK(b[i] >= a[i]);
					if (!touches[lab.at<int>(y, x)]) CHECK(a[i] == b[i]);
					if (a[i] != b[i]) { px_diff++; any = true; }
				}
			masks_diff += any;
		}
		printf("visibility-mask regions, 300 random masks: %lld of %lld pixels (%lld masks) differ from the reference model, all in regions touching the last row/column\n", px_diff, px_total, masks_diff);
	}
	// a truncated BinMat must be rejected and leave the destination untouched
	{
		Mat d(8, 8, CV_32FC1);
		std::memset(d.data, 0, d.step * d.rows);
		CHECK(WriteBinMat(tmp / "t_trunc.dmb", d));
		std::filesystem::resize_file(tmp / "t_trunc.dmb", 16 + 100);
		Mat keep(2, 2, CV_8UC1);
		CHECK(!ReadBinMat(tmp / "t_trunc.dmb", keep));
		CHECK(keep.rows == 2 && keep.cols == 2 && keep.type() == CV_8UC1);
		std::ofstream bad(tmp / "t_badhdr.dmb", std::ios::binary);
		const int32_t h[4] = { 1, -3, 7, 5 };
		bad.write((const char*)h, 16);
		bad.close();
		CHECK(!ReadBinMat(tmp / "t_badhdr.dmb", keep));
	}
	// rescale helpers
	{
		Mat a(4, 6, CV_32FC1);
		for (int r = 0; r < 4; ++r) for (int c = 0; c < 6; ++c) a.at<float>(r, c) = (float)(r * 6 + c);
		Mat same = ResizeLinear(a, 6, 4);
		CHECK(std::memcmp(same.data, a.data, 4 * 6 * 4) == 0);
		Mat half = ResizeLinear(a, 3, 2);
		CHECK(half.rows == 2 && half.cols == 3);
		CHECK(std::fabs(half.at<float>(0, 0) - 3.5f) < 1e-5f);   // mean of the 2x2 block {0,1,6,7}
		Mat up;
		RescaleMatToTargetSize<float>(a, up, 12, 8);
		CHECK(up.rows == 8 && up.cols == 12 && up.at<float>(0, 0) == 0.0f && up.at<float>(7, 11) == a.at<float>(3, 5));
	}
	// PLY header (APD.cpp:842-882)
	{
		std::vector<PointList> pc(2);
		pc[0].coord = float3{1, 2, 3}; pc[0].color = float3{10, 20, 30};
		pc[1].coord = float3{4, 5, 6}; pc[1].color = float3{40, 50, 60};
		CHECK(ExportPointCloud(tmp / "t.ply", pc));
		std::ifstream f(tmp / "t.ply", std::ios::binary);
		std::string l;
		std::getline(f, l); CHECK(l == "ply");
		std::getline(f, l); CHECK(l == "format binary_little_endian 1.0");
		std::getline(f, l); CHECK(l == "element vertex 2");
		int lines = 3;
		while (std::getline(f, l)) { lines++; if (l == "end_header") break; }
		CHECK(lines == 10);
		std::vector<char> rest((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
		CHECK(rest.size() == 2 * 15);
	}
	// Canny edge front end (EdgeSegment mode 0): a vertical step must give one thin vertical edge
	{
		Mat img(40, 60, CV_8UC1);
		for (int r = 0; r < 40; ++r) for (int c = 0; c < 60; ++c) img.at<uint8_t>(r, c) = c < 30 ? 60 : 180;
		Mat e = EdgeSegment(0, img, 0, true);
		CHECK(e.rows == 40 && e.cols == 60);
		int on_step = 0, elsewhere = 0;
		for (int r = 2; r < 38; ++r)
			for (int c = 0; c < 60; ++c)
				if (e.at<uint8_t>(r, c)) { if (c == 29 || c == 30) on_step++; else elsewhere++; }
		CHECK(on_step == 36 && elsewhere == 0);
		Mat flat = Mat::zeros(20, 20, CV_8UC1);
		Mat e2 = EdgeSegment(0, flat, 0, true);
		int any = 0;
		for (int i = 0; i < 400; ++i) any += e2.data[i];
		CHECK(any == 0);
	}
	// Delaunay substitute of cv::Subdiv2D (APD.cpp:51-80): empty-circumcircle property + coverage
	{
		std::vector<float2> pts;
		std::vector<float> rates;
		uint32_t lcg = 12345u;
		auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) * (1.0f / 16777216.0f); };
		for (int i = 0; i < 300; ++i) { pts.push_back(float2{ 10.0f + 180.0f * rnd(), 10.0f + 130.0f * rnd() }); rates.push_back((float)i); }
		pts.push_back(pts[7]); rates.push_back(1000.0f);            // duplicate position: ignored, last rate wins
		pts.push_back(float2{ -5.0f, 20.0f }); rates.push_back(0);   // outside: not inserted
		const Rect rc(0, 0, 200, 150);
		auto tris = DelaunayTriangulation(200, 150, rc, pts, rates);
		int real = 0, saw_dup_rate = 0;
		for (const auto& t : tris) {
			if (!(rc.contains(t.pt1) && rc.contains(t.pt2) && rc.contains(t.pt3))) continue;
			real++;
			if (t.rate1 == 1000.0f || t.rate2 == 1000.0f || t.rate3 == 1000.0f) saw_dup_rate = 1;
			CHECK(t.rate1 != 7.0f && t.rate2 != 7.0f && t.rate3 != 7.0f);
		}
		CHECK(real > 500 && real < 600 && saw_dup_rate);   // ~2n - 2 - hull
		// recompute with exact float vertices to test the Delaunay property
		// (triangle corners are truncated to int in the API, so rebuild from rates = point index)
		for (const auto& t : tris) {
			if (!(rc.contains(t.pt1) && rc.contains(t.pt2) && rc.contains(t.pt3))) continue;
			auto idx = [&](float r) { return r == 1000.0f ? 7 : (int)r; };
			const float2 a = pts[idx(t.rate1)], b = pts[idx(t.rate2)], c = pts[idx(t.rate3)];
			CHECK((int)a.x == t.pt1.x && (int)a.y == t.pt1.y && (int)c.x == t.pt3.x);
			const double bx = (double)b.x - a.x, by = (double)b.y - a.y, cx = (double)c.x - a.x, cy = (double)c.y - a.y;
			const double d = 2.0 * (bx * cy - by * cx);
			CHECK(std::fabs(d) > 1e-9);
			const double ux = (cy * (bx * bx + by * by) - by * (cx * cx + cy * cy)) / d;
			const double uy = (bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by)) / d;
			const double r2 = ux * ux + uy * uy;
			for (int k = 0; k < 300; ++k) {
				const double dx = pts[k].x - (a.x + ux), dy = pts[k].y - (a.y + uy);
				CHECK(dx * dx + dy * dy > r2 * (1.0 - 1e-9));
			}
		}
	}
	// Depth-Anything prior (APD.cpp:1210-1424): relative map + sparse points -> metric depth -> planes
	{
		const int W = 160, H = 120;
		Camera cam{};
		const float K[9] = { 150, 0, 80, 0, 150, 60, 0, 0, 1 };
		const float ang = 0.3f;
		const float R[9] = { std::cos(ang), 0, std::sin(ang), 0, 1, 0, -std::sin(ang), 0, std::cos(ang) };
		std::memcpy(cam.K, K, sizeof K);
		std::memcpy(cam.R, R, sizeof R);
		cam.t[0] = 0.1f; cam.t[1] = -0.2f; cam.t[2] = 0.3f;
		for (int j = 0; j < 3; ++j) cam.c[j] = -(R[j] * cam.t[0] + R[3 + j] * cam.t[1] + R[6 + j] * cam.t[2]);
		cam.width = W; cam.height = H;
		// camera-frame plane n.X = dplane
		const float n[3] = { 0.2f, -0.1f, -0.9746794f };
		const float dplane = -4.0f;
		auto depth_at = [&](float x, float y) { return dplane / (n[0] * (x - K[2]) / K[0] + n[1] * (y - K[5]) / K[4] + n[2]); };
		Mat raw(H, W, CV_32FC1), truth(H, W, CV_32FC1);
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x) {
				truth.at<float>(y, x) = depth_at((float)x, (float)y);
				const float s = 20.0f * (1.0f + 0.001f * x + 0.0005f * y);   // relative-to-metric ratio, linear over the image
				raw.at<float>(y, x) = 255.0f - s * truth.at<float>(y, x);
			}
		std::vector<float2> xy;
		std::vector<float3> xyz;
		uint32_t lcg = 99u;
		auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) * (1.0f / 16777216.0f); };
		for (int i = 0; i < 400; ++i) {
			const int px = 2 + (int)(rnd() * (W - 4)), py = 2 + (int)(rnd() * (H - 4));
			const float Z = depth_at((float)px, (float)py);
			const float Xc[3] = { Z * (px - K[2]) / K[0], Z * (py - K[5]) / K[4], Z };
			float3 Xw;   // X_world = R^T (X_cam - t)
			const float e[3] = { Xc[0] - cam.t[0], Xc[1] - cam.t[1], Xc[2] - cam.t[2] };
			Xw.x = R[0] * e[0] + R[3] * e[1] + R[6] * e[2];
			Xw.y = R[1] * e[0] + R[4] * e[1] + R[7] * e[2];
			Xw.z = R[2] * e[0] + R[5] * e[1] + R[8] * e[2];
			xy.push_back(float2{ (float)px, (float)py });
			xyz.push_back(Xw);
		}
		float2 pp; float pd;
		ProjectCamera(xyz[0], cam, pp, pd);
		CHECK(std::fabs(pp.x - xy[0].x) < 1e-2f && std::fabs(pp.y - xy[0].y) < 1e-2f);
		Mat dep = raw.clone();
		CHECK(MetricDepthFromPrior(dep, xy, xyz, cam));
		int good = 0, inside = 0;
		for (int y = 30; y < H - 30; ++y)
			for (int x = 30; x < W - 30; ++x) {
				inside++;
				if (std::fabs(dep.at<float>(y, x) / truth.at<float>(y, x) - 1.0f) < 2e-3f) good++;
			}
		// the reference's sweep (truncating pixel casts + unsigned-area barycentric weights,
		// APD.cpp:1333-1347, 30-49) extrapolates badly along sliver triangles and can miss isolated
		// pixels (those keep rates[n/2]): streaks of wrong ratios are its behaviour, reproduced here
		CHECK(good >= inside * 0.75);
		std::vector<float4> planes((size_t)W * H);
		PlanesFromDepth(truth, cam, planes.data());
		const float nw[3] = { R[0] * n[0] + R[3] * n[1] + R[6] * n[2], R[1] * n[0] + R[4] * n[1] + R[7] * n[2], R[2] * n[0] + R[5] * n[1] + R[8] * n[2] };
		for (int y = 1; y < H - 1; y += 7)
			for (int x = 1; x < W - 1; x += 5) {
				const float4 p = planes[(size_t)y * W + x];
				CHECK(std::fabs(p.x - nw[0]) < 2e-3f && std::fabs(p.y - nw[1]) < 2e-3f && std::fabs(p.z - nw[2]) < 2e-3f);
				CHECK(p.w == truth.at<float>(y, x));
			}
		CHECK(planes[0].x == 0 && planes[0].w == truth.at<float>(0, 0));
		Mat empty;
		CHECK(!MetricDepthFromPrior(empty, xy, xyz, cam));
		Mat dep2 = raw.clone();
		CHECK(!MetricDepthFromPrior(dep2, {}, {}, cam));
	}
	static_assert(sizeof(Camera) == 112 && sizeof(PatchMatchParams) == 76, "POD layouts");
	printf("host tests ok\n");
	return 0;
}
