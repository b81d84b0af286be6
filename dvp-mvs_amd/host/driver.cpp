// driver.cpp — what of the driver runs without a GPU: the command line of `apd <dense_folder>`, the coarse-to-fine pass list (/root/reference/main.cpp:421-528), the host's visibility clean-up
#include "driver.h"

const char* const kApdUsage = "USAGE: apd dense_folder [gpu_index] [--previews] [--max-src N] [--iters N] [--min-scale S] [--passes P] [--seed X] [--rank R --world N [--job ID]] [--jacobi] [--no-fusion | --fusion KIND] [--fusion-on device|host] [--edges-on host|gpu] [--labels-on host|gpu] [--cleanup-on host|gpu] [--images-on host|gpu] [--prior-on host|gpu] [--decode-on host|gpu] [--strong-wide on|off] [--views-in-flight N]\n";

// (kept out of kApdUsage: tests/test_driver_host.py pins the options that text names)
const char* const kApdEntropyUsage = "USAGE: --entropy-on host|gpu moves the input JPEGs' Huffman decode to the device and takes effect only together with --decode-on gpu: apd dense_folder --decode-on gpu --entropy-on gpu\n";

// `--X first|second`: whether the word is the second one; any other word ends the process
static bool SecondWord(const std::string& option, const std::string& word, const char* first, const char* second) {
	if (word != first && word != second) { std::cerr << option << " takes " << first << " or " << second << "\n"; std::exit(1); }
	return word == second;
}

Options ParseOptions(int argc, char** argv) {
	static const std::pair<const char*, bool RunConfig::*> on_gpu[] = {
		{ "--edges-on", &RunConfig::edges_on_device }, { "--labels-on", &RunConfig::labels_on_device }, { "--prior-on", &RunConfig::prior_on_device },
		{ "--cleanup-on", &RunConfig::cleanup_on_device }, { "--decode-on", &RunConfig::decode_on_device }, { "--images-on", &RunConfig::images_on_device },
		{ "--entropy-on", &RunConfig::entropy_on_device } };
	Options o;
	o.dense_folder = argv[1];
	int a = 2;
	if (argc > 2 && argv[2][0] != '-') { o.gpu = std::atoi(argv[2]); a = 3; }
	for (; a < argc; ++a) {
		const std::string s = argv[a];
		auto val = [&]() { return (a + 1 < argc) ? std::atoll(argv[++a]) : 0ll; };
		bool RunConfig::* where = nullptr;
		for (const auto& f : on_gpu)
			if (s == f.first) where = f.second;
		if (where) { if (a + 1 < argc) o.run.*where = SecondWord(s, argv[++a], "host", "gpu"); }
		else if (s == "--strong-wide") { if (a + 1 < argc) o.run.strong_wide = !SecondWord(s, argv[++a], "on", "off"); }
		else if (s == "--max-src") o.max_src = (int)val();
		else if (s == "--iters") o.iters = (int)val();              // the reference hard-wires 3 (main.cpp:476,502)
		else if (s == "--min-scale") o.min_scale = (int)val();      // the reference stops at half resolution (main.cpp:450,456)
		else if (s == "--passes") o.geom_passes = (int)val();       // REFINE_ITER passes per level (3 in the reference)
		else if (s == "--seed") o.seed = (uint64_t)val();
		else if (s == "--rank") o.rank = (int)val();
		else if (s == "--world") o.world = (int)val();
		else if (s == "--job") { if (a + 1 < argc) o.job = argv[++a]; }
		else if (s == "--transport") { if (a + 1 < argc) o.transport = argv[++a]; }
		else if (s == "--collective-timeout") o.collective_timeout_s = (int)val();
		else if (s == "--jacobi") o.jacobi = true;
		else if (s == "--labels") o.run.use_label_files = true;
		else if (s == "--no-fusion") o.fusion = false;
		else if (s == "--sync-io") o.sync_io = true;
		else if (s == "--views-in-flight") { if (a + 1 < argc) o.views_in_flight = std::min(APD::kMaxViewsInFlight, std::max(1, atoi(argv[++a]))); }   // one pooled engine context per view in flight
		else if (s == "--in-flight-pixels") { if (a + 1 < argc) o.in_flight_pixels = atoll(argv[++a]); }
		else if (s == "--previews") o.previews = true;
		else if (s == "--host-rescale") o.host_rescale = true;
		else if (s == "--fusion") { if (a + 1 < argc) o.fusion_kind = argv[++a]; }
		else if (s == "--fusion-on") { if (a + 1 < argc) o.fusion_on_host = std::string(argv[++a]) == "host"; }   // device (default) | host
	}
	if (o.run.entropy_on_device && !o.run.decode_on_device) { std::cerr << kApdEntropyUsage; std::exit(1); }
	o.run.device_rescale = o.run.device_maps = !o.sync_io && !o.host_rescale;
	if (o.world > 1) o.jacobi = true;
	if (o.job.empty())   // a launcher-provided id; with --world > 1 RankComm refuses to start without one
		for (const char* e : { "DVP_JOB_ID", "TORCHELASTIC_RUN_ID", "SLURM_JOB_ID" })
			if (const char* v = std::getenv(e)) { o.job = v; break; }
	return o;
}

std::vector<Pass> BuildPlan(int round_num, int min_scale, int geom_passes) {
	std::vector<Pass> plan;
	for (int level = 0; level < round_num; ++level) {
		const int scale = 1 << (round_num - 1 - level);
		if (scale < min_scale && round_num != 1) break;
		plan.push_back(Pass{ level, scale, -1 });
		for (int j = 0; j < geom_passes; ++j) plan.push_back(Pass{ level, scale, j });
	}
	return plan;
}

void ConfigurePass(Problem& problem, const Pass& pass, int iteration, int iters, int round_num) {
	PatchMatchParams& q = problem.params;
	problem.iteration = iteration;
	problem.scale_size = pass.scale;
	q.max_iterations = iters;
	if (pass.level > 0 || pass.geom_index >= 0) {
		q.ransac_threshold = (float)(0.01 - pass.level * 0.00125);
		q.rotate_time = std::min(static_cast<int>(std::pow(2, pass.level)), 4);
	}
	if (pass.geom_index < 0) {
		q.state = pass.level == 0 ? FIRST_INIT : REFINE_INIT;
		q.use_APD = pass.level != 0;
		// main.cpp:465-470: on below the finest pyramid level only (the reference never runs the finest one; with
		// --min-scale 1 its own rule, i < round_num - 1, leaves use_detail off there)
		if (pass.level != 0) q.use_detail = pass.level < round_num - 1;
		q.geom_consistency = false;
		q.weak_peak_radius = 6;
	} else {
		q.state = REFINE_ITER;
		q.use_APD = pass.level != 0;
		q.geom_consistency = true;
		q.weak_peak_radius = std::max(4 - 2 * pass.geom_index, 2);
	}
}

// ProcessProblem's visibility clean-up (main.cpp:311-363) on the selected-view words of a view (what `apd --cleanup-on host`
// runs): per source view, every 4-connected region of pixels that do NOT select the view and is smaller than min_region
// pixels is switched to "selected".  Bits at and above nsrc come out clear.
void CleanSelectedViewsOnHost(Mat& views, int nsrc, int min_region) {
	const int width = views.cols, height = views.rows;
	std::vector<Mat> fill(nsrc);   // per source: 1 where the bit has to be set
#pragma omp parallel for schedule(dynamic, 1) num_threads(nsrc < 8 ? (nsrc > 0 ? nsrc : 1) : 8)
	for (int i = 0; i < nsrc; ++i) {
		Mat visible(height, width, CV_8UC1);
		for (int r = 0; r < height; ++r) {
			const uint32_t* w = views.ptr<uint32_t>(r);
			uint8_t* v = visible.ptr<uint8_t>(r);
			for (int c = 0; c < width; ++c) v[c] = ((w[c] >> i) & 1u) ? 255 : 0;
		}
		Mat region(height, width, CV_32S);
		std::vector<int> region_size;
		Connect(visible, region, region_size);
		Label_Update(region, region_size);
		fill[i] = Mat(height, width, CV_8UC1);
		for (int r = 0; r < height; ++r) {
			const int* lab = region.ptr<int>(r);
			uint8_t* f = fill[i].ptr<uint8_t>(r);
			for (int c = 0; c < width; ++c) f[c] = (lab[c] != 0 && region_size[lab[c]] >= min_region) ? 0 : 1;
		}
	}
#pragma omp parallel for schedule(static) num_threads(HostThreads())
	for (int r = 0; r < height; ++r) {
		uint32_t* w = views.ptr<uint32_t>(r);
		for (int c = 0; c < width; ++c) {
			unsigned int mask = 0;
			for (int i = 0; i < nsrc; ++i) mask |= (unsigned int)fill[i].at<uint8_t>(r, c) << i;
			w[c] = mask;                      // APD.SetPixelSelectedViews(r, c, mask)
		}
	}
}
