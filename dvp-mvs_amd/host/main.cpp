// main.cpp — the driver: the reference's coarse-to-fine schedule (/root/reference/main.cpp:421-528) over
// `class APD`, one process per GPU.  Three forms:
//   apd <dense_folder> [gpu_index] [options]: kApdUsage and ParseOptions (host/driver.cpp)
//   apd --convert-from <colmap folder> <save folder> [options]: ConvertMain below
//       the reference's colmap2mvsnet.py: a COLMAP model -> the folder the first form reads (host/colmap.cpp)
//   apd --evaluate <recon.ply> --against <truth.ply> [options]: EvaluateMain below
//       accuracy, completeness and F1 of a fused cloud against a ground-truth cloud (host/evaluate.cpp)
//
// Schedule.  The image pyramid has round_num levels (the longer side is halved until <= 800).  Level i
// runs one "A" pass without geometric consistency — FIRST_INIT from scratch / the Depth-Anything prior
// at the coarsest level, REFINE_INIT from the up-sampled result of the level below otherwise — and then
// `passes` REFINE_ITER passes with geometric consistency against the source views' depth maps.  The
// reference stops before the finest level (`i < round_num - 1`); --min-scale 1 adds it.
//
// Multi-GPU.  Views of a pass are independent: view v belongs to rank v % world.  Every rank decodes and
// resizes the images of ITS views at a level and broadcasts them (RCCL), so that the decode work scales with the
// rank count and every file is read once; after every pass each view's new depth map is
// broadcast by its owner and kept resident on every GPU, which is where the next pass' geometric term
// reads it (Jacobi: a pass sees the previous pass' maps only).  --job must be unique per run (default: $DVP_JOB_ID,
// $TORCHELASTIC_RUN_ID or $SLURM_JOB_ID); a rank that fails takes the whole job down (comm.h, "Failure model").  With one rank the default is the
// reference's in-place order (a view sees the maps its predecessors wrote in the same pass, through the
// result files); --jacobi selects the exchange semantics there too, which makes a run independent of the
// number of ranks.  Result files are always written to a temporary name and renamed, so a reader never
// sees a torn file.
#include "driver.h"
#include <thread>
#include "comm.h"
#include "colmap.h"
#include "evaluate.h"
#include <map>
#include <set>
#include <memory>
#include <future>
#include <mutex>

namespace {

// pair.txt (written by colmap2mvsnet.py:442-448; read at main.cpp:127-170): a whitespace-separated
// stream — the number of views, then per view its id, the number of candidates k and k (id, score)
// pairs.  Candidates with a non-positive score are dropped; at most `max_src` are kept (0 = all).
std::vector<Problem> ReadViewGraph(const path& dense_folder, int max_src) {
	std::vector<Problem> problems;
	std::ifstream in(dense_folder / "pair.txt");
	int n_views = 0;
	if (!(in >> n_views)) return problems;
	for (int i = 0; i < n_views; ++i) {
		Problem p;
		int k = 0;
		if (!(in >> p.ref_image_id >> k)) break;
		p.index = i;
		p.dense_folder = dense_folder;
		p.result_folder = dense_folder / "APD" / ToFormatIndex(p.ref_image_id);
		for (int j = 0; j < k; ++j) {
			int id = 0;
			float score = 0.0f;
			in >> id >> score;
			if (score > 0.0f && (max_src <= 0 || (int)p.src_image_ids.size() < max_src)) p.src_image_ids.push_back(id);
		}
		std::filesystem::create_directories(p.result_folder);
		problems.push_back(std::move(p));
	}
	return problems;
}

int LevelsOf(int cols, int rows) {   // main.cpp:248-264
	int levels = 1;
	for (int side = std::max(cols, rows); side > 800; side /= 2) ++levels;
	return levels;
}
int PyramidLevels(const std::vector<Problem>& problems) {
	if (problems.empty()) return 0;
	const Mat first = APD::DecodedGray(problems[0].dense_folder / "images" / (ToFormatIndex(problems[0].ref_image_id) + ".jpg"));
	return first.empty() ? 0 : LevelsOf(first.cols, first.rows);
}

// View -> rank.  Round 4 dealt the views round-robin (v % world).  Views differ in cost — by their pixel count when the images
// of a folder differ in size (APD.cpp:1071-1079 allows it), by their WEAK share (one WEAK pixel costs ~4 others) —, and a pass
// ends when its busiest rank does: longest-predicted-first instead (the view with the largest predicted cost goes to the rank
// with the least load so far; ties: lower view index, lower rank).  Predicted cost = the view's pixels (from the file header:
// every rank computes the same table without decoding anything); the assignment holds for the whole job, so a view's
// maps of the previous pass stay in its owner's result cache.  Equal-size views: the same table as v % world.
// tools/scale_sim.py predicts what the policy is worth.
std::vector<int> AssignViews(const std::vector<Problem>& problems, int world) {
	std::vector<int> owner(problems.size(), 0);
	if (world <= 1) return owner;
	std::vector<std::pair<long long, int>> cost;   // (-pixels, view): ascending sort = largest first, lower index first
	for (const Problem& p : problems) {
		int w = 0, h = 0;
		if (!ImageFileSize(p.dense_folder / "images" / (ToFormatIndex(p.ref_image_id) + ".jpg"), &w, &h)) { w = 1; h = 1; }   // unreadable: the owner will stop the job (DvpFatal) when it loads it
		cost.emplace_back(-(long long)w * h, p.index);
	}
	std::sort(cost.begin(), cost.end());
	std::vector<long long> load((size_t)world, 0);
	for (const auto& c : cost) {
		int best = 0;
		for (int r = 1; r < world; ++r)
			if (load[(size_t)r] < load[(size_t)best]) best = r;
		owner[(size_t)c.second] = best;
		load[(size_t)best] += -c.first;
	}
	return owner;
}

// What a finished view hands to the background worker: its maps (the fetch functions fill the staged ones), the fetches that
// are still to run, and what the publishing needs to know of the view
struct ViewJob {
	path folder;
	int iteration = 0, nsrc = 0, min_region = 0;
	bool previews = false;
	bool cleaned_on_device = false;   // --cleanup-on gpu: the engine cleaned the staged words (RunConfig::cleanup_on_device); flows without staged maps keep the host loop
	Mat depth, normal, pixel_states, views, radius;
	std::function<void()> fetch_edge, fetch_maps;
	std::function<std::vector<std::vector<uint8_t>>()> fetch_previews;
	std::vector<std::vector<uint8_t>> preview_files;
};

void BackgroundLap(const char* what, std::chrono::steady_clock::time_point t0) {
	if (!HostTiming()) return;   // (one write per line: the driver threads print their views' blocks meanwhile)
	std::ostringstream line;
	line << "  [background] " << what << ": " << std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() / 1000.0 << " ms\n";
	std::cout << line.str() << std::flush;
}

// The view's background job.  The depth map is what OTHER views read next: it was published (or announced) by ProcessProblem.
// Everything else — the visibility clean-up and the remaining four files — is only read by this view's own next pass.
void FinishView(ViewJob& j) {
	const auto t0 = std::chrono::steady_clock::now();
	if (j.fetch_edge) j.fetch_edge();
	if (j.fetch_previews) j.preview_files = j.fetch_previews();
	if (j.fetch_maps) {
		j.fetch_maps();
		PublishResult(j.folder / "depths.dmb", j.depth);
		BackgroundLap("maps to the host", t0);
	}
	if (j.cleaned_on_device) std::cout << "Visibility clean-up: on the device\n" << std::flush;   // (the words fetched above are final)
	else {
		// DVP_RAW_VIEWS_DIR=<dir> (host clean-up only): the words as the pass left them, <dir>/<view folder>_<iteration>.bin, so that
		// a test can tell whether the clean-up had anything to do
		if (const char* raw_dir = std::getenv("DVP_RAW_VIEWS_DIR")) {
			const path file = path(raw_dir) / (j.folder.filename().string() + "_" + std::to_string(j.iteration) + ".bin");
			if (!j.views.empty() && !WriteFileAtomic(file, j.views.ptr<uint8_t>(0), j.views.total() * 4)) DvpFatal("cannot write " + file.string());
		}
		CleanSelectedViewsOnHost(j.views, j.nsrc, j.min_region);
	}
	PublishResult(j.folder / "APD_normals.dmb", j.normal);
	PublishResult(j.folder / "weak.bin", j.pixel_states);
	PublishResult(j.folder / "selected_views.bin", j.views);
	if (!j.radius.empty()) PublishResult(j.folder / "radius.bin", j.radius);
	if (j.iteration == 15 || j.iteration == Run().final_iteration) {   // main.cpp:378-384
		writeDepthDmb(j.folder / "depths_geom.dmb", j.depth);
		writeNormalDmb(j.folder / "normals.dmb", j.normal);
		if (j.previews && !WriteWeakPng(j.folder / "weak.png", j.pixel_states)) DvpFatal("cannot write " + (j.folder / "weak.png").string());
	}
	const char* preview_names[3] = { "depth_", "normal_", "weak_" };   // ShowDepthMap / ShowNormalMap / ShowWeakImage, main.cpp:396-403
	for (size_t i = 0; i < j.preview_files.size(); ++i) {
		const path file = j.folder / (preview_names[i] + std::to_string(j.iteration) + ".jpg");
		if (!WriteFileAtomic(file, j.preview_files[i].data(), j.preview_files[i].size())) DvpFatal("cannot write " + file.string());
	}
	BackgroundLap("visibility-mask clean-up + publish", t0);
}

// planes -> depth / normal maps on the host (flows without staged maps); depths outside the admissible range are dropped and
// the pixel loses its state (main.cpp:300-309)
void UnpackPlanesOnHost(APD& APD, Mat& depth, Mat& normal, Mat& pixel_states) {
	const int width = APD.GetWidth(), height = APD.GetHeight();
	const float dmin = APD.GetDepthMin(), dmax = APD.GetDepthMax();
	depth = Mat(height, width, CV_32FC1);
	normal = Mat(height, width, CV_32FC3);
#pragma omp parallel for schedule(static) num_threads(HostThreads())
	for (int r = 0; r < height; ++r) {
		float* z = depth.ptr<float>(r);
		Vec3f* n = normal.ptr<Vec3f>(r);
		uint8_t* st = pixel_states.ptr<uint8_t>(r);
		for (int c = 0; c < width; ++c) {
			const float4 ph = APD.GetPlaneHypothesis(r, c);
			n[c] = Vec3f{ ph.x, ph.y, ph.z };
			const bool usable = !(ph.w < dmin || ph.w > dmax);
			z[c] = usable ? ph.w : 0.0f;
			if (!usable) st[c] = UNKNOWN;
		}
	}
}

// DVP_HOST_TIMING: where the GPU time of the view went, launch site by launch site (event pairs around each site: gaps between
// sites — a host that is late with the next launch — show as the difference to the total)
void LogGpuSites(const DvpTimings& t, int image_format) {
	static const char* names[DVP_ST_COUNT] = { "gen_edge_inform", "find_nearest_strong", "gen_neighbours", "neighbour_update", "random_init", "strong_update", "ransac_fit", "weak_update", "get_depth_normal", "filter_strong", "depth_to_weak", "local_refine", "strong_prep" };
	double sum = 0.0;
	ViewLog() << "  [gpu]";
	for (int i = 0; i < DVP_ST_COUNT; ++i)
		if (t.stage_ms[i] > 0.0) { ViewLog() << " " << names[i] << " " << t.stage_ms[i]; sum += t.stage_ms[i]; }
	static const char* formats[3] = { "f32", "u8", "f16" };   // the image planes the weak update read (dvp_image_format)
	ViewLog() << " | sites " << sum << " of total " << t.total_ms << " ms | images " << formats[image_format >= 0 && image_format <= 2 ? image_format : 0] << std::endl;
}

struct ViewResult { Mat depth; };   // what the exchange step needs from a finished view
// `resident_depth(w, h)`: where on the device the view's new depth map goes for the views that read it as a source (or null)
ViewResult ProcessProblem(const Problem& problem, const std::function<float*(int, int)>& resident_depth = nullptr) {   // main.cpp:267-419
	ViewLog() << "Processing image: " << std::setw(8) << std::setfill('0') << problem.ref_image_id << "..." << std::endl;
	ViewLog() << "Iteration: " << problem.iteration << std::endl;
	const auto start = std::chrono::steady_clock::now();
	Lap lap{ "  [host] ", start };   // wall time of every host step of the view (where the non-GPU time goes)
	APD APD(problem);
	APD.InuputInitialization();
	lap("InuputInitialization (images, cameras, previous results)");
	APD.SupportInitialization();
	lap("SupportInitialization (edges, labels, radius)");
	APD.CudaSpaceInitialization();
	lap("CudaSpaceInitialization (context + uploads)");
	APD.SetDataPassHelperInCuda();
	const int width = APD.GetWidth(), height = APD.GetHeight();
	ViewJob job;
	job.folder = problem.result_folder;
	job.iteration = problem.iteration;
	job.nsrc = (int)problem.src_image_ids.size();
	job.min_region = 20 * (8 / problem.scale_size) * (8 / problem.scale_size);   // main.cpp:311-363: regions smaller than 20 * (8 / scale)^2 pixels are filled
	job.previews = problem.show_medium_result;
	if (Run().device_maps) job.fetch_maps = APD.RunPatchMatchAndStageMaps(job.depth, job.normal, resident_depth ? resident_depth(width, height) : nullptr);
	else APD.RunPatchMatch();
	// previews (main.cpp:396-403): rendered and encoded from the context's planes right after the maps were staged; fetched by
	// the background job before it fetches the maps (or here, when there are no staged maps and the context may be gone
	// before the job runs)
	if (job.previews) job.fetch_previews = APD.BeginPreviews();
	if (job.fetch_previews && !job.fetch_maps) { job.preview_files = job.fetch_previews(); job.fetch_previews = nullptr; }
	// --edges-on gpu: the edge map the engine made for this view is fetched and published as edges_<s>.dmb by the background
	// job, or here when that job may run after the context is gone
	job.fetch_edge = APD.TakeEdgeFetch();
	if (job.fetch_edge && !job.fetch_maps) { job.fetch_edge(); job.fetch_edge = nullptr; }
	if (Run().strong_wide && job.nsrc > 16 && APD.GetStrongUpdateForm() != 0) ViewLog() << "Strong update: split form, " << job.nsrc << " views" << std::endl;
	lap(Run().device_maps ? "RunPatchMatch" : "RunPatchMatch + download");
	job.pixel_states = APD.GetPixelStates();
	job.views = APD.GetSelectedViews();
	job.radius = problem.params.use_radius ? APD.GetRadiusMap() : Mat();
	if (!Run().device_maps) UnpackPlanesOnHost(APD, job.depth, job.normal, job.pixel_states);
	lap("unpack planes");
	// The depth map is published now; the rest of the view's files are announced and follow from the background job, which runs
	// while the GPU is already on the next view (store.cpp).
	if (job.fetch_maps) ExpectResult(job.folder / "depths.dmb");   // (a reader of the file waits for the job below; same-size views take the device copy)
	else PublishResult(job.folder / "depths.dmb", job.depth);
	for (const char* name : { "APD_normals.dmb", "weak.bin", "selected_views.bin" }) ExpectResult(job.folder / name);
	if (problem.params.use_radius) ExpectResult(job.folder / "radius.bin");
	job.cleaned_on_device = job.fetch_maps && Run().cleanup_on_device;
	const ViewResult result{ job.depth };
	RunInBackground([job = std::move(job)]() mutable { FinishView(job); });
	lap("hand-over to the background worker");
	const auto end = std::chrono::steady_clock::now();
	const DvpTimings& t = APD.GetTimings();
	ViewLog() << "Processing image: " << std::setw(8) << std::setfill('0') << problem.ref_image_id << " done!" << std::endl;
	if (HostTiming()) LogGpuSites(t, APD.GetImageFormat());
	ViewLog() << "Cost time: " << std::chrono::duration_cast<std::chrono::milliseconds>(end - start).count() << " ms (GPU RunPatchMatch "
	          << t.total_ms << " ms, " << (double)width * height * problem.params.max_iterations / (t.total_ms * 1e3) << " Mpx/s/iter)" << std::endl;
	return result;
}

// depth maps of every view, resident on this rank's device, refreshed after each pass.  Views may differ in size
// (the reference pads / crops source images and rescales source depth maps, APD.cpp:1071-1079, 1147-1166): every
// map travels with its own dimensions.
class DepthExchange {
public:
	DepthExchange(RankComm& comm, const std::vector<Problem>& problems, const std::vector<int>& owner) : comm_(comm), problems_(problems), owner_(owner) {}
	~DepthExchange() { Release(); }
	// `mine`: view index -> the depth map this rank computed in the pass just finished
	void Publish(const std::map<int, Mat>& mine) {
		// agreed check first: a rank that lacks one of its maps must not leave the others inside a collective
		bool ok = true;
		for (size_t v = 0; v < problems_.size(); ++v)
			if (owner_[v] == comm_.rank() && (mine.find((int)v) == mine.end() || mine.at((int)v).empty())) ok = false;
		if (!comm_.AllOk(ok)) {
			std::cerr << "DepthExchange: a rank is missing a depth map of the pass" << std::endl;
			if (comm_.world() > 1) comm_.Abort("DepthExchange: missing depth map");
			exit(EXIT_FAILURE);
		}
		for (size_t v = 0; v < problems_.size(); ++v) {
			const int owner = owner_[v];
			int dims[2] = { 0, 0 };
			if (owner == comm_.rank()) { dims[0] = mine.at((int)v).cols; dims[1] = mine.at((int)v).rows; }
			comm_.BroadcastHost(dims, sizeof(dims), owner);
			Slot& s = maps_[problems_[v].ref_image_id];
			const size_t count = (size_t)dims[0] * dims[1];
			if (s.w != dims[0] || s.h != dims[1]) {
				RankComm::DeviceFree(s.dev);
				s.dev = RankComm::DeviceAlloc(count);
				s.w = dims[0];
				s.h = dims[1];
			}
			if (owner == comm_.rank()) RankComm::HostToDevice(s.dev, mine.at((int)v).ptr<float>(0), count);
			comm_.BroadcastDevice(s.dev, count, owner);
			APD::SetResidentDepth(problems_[v].ref_image_id, s.dev, s.w, s.h);
		}
	}
	void Release() {
		APD::ClearResidentDepths();
		for (auto& kv : maps_) RankComm::DeviceFree(kv.second.dev);
		maps_.clear();
	}
private:
	struct Slot { float* dev = nullptr; int w = 0, h = 0; };
	RankComm& comm_;
	const std::vector<Problem>& problems_;
	const std::vector<int>& owner_;
	std::map<int, Slot> maps_;
};

// Single-rank, in-place order (the reference's): a finished view's depth map goes to the device right away and stays
// there, so that the views after it — which see it as a source map in the same pass, exactly as they would through
// APD/<id>/depths.dmb — take it with a device-to-device copy instead of a 100 MB file read + upload per source.
class InPlaceDepths {
public:
	~InPlaceDepths() { Release(); }
	void Update(int image_id, const Mat& depth) {
		Slot& s = maps_[image_id];
		if (s.w != depth.cols || s.h != depth.rows) {
			APD::UnsetResidentDepth(image_id);   // the registry must not name a freed block, not even until the new one is registered
			RankComm::DeviceFree(s.dev);
			s.dev = RankComm::DeviceAlloc((size_t)depth.cols * depth.rows);
			s.w = depth.cols;
			s.h = depth.rows;
		}
		RankComm::HostToDevice(s.dev, depth.ptr<float>(0), (size_t)s.w * s.h);
		APD::SetResidentDepth(image_id, s.dev, s.w, s.h);
	}
	// ... or straight from the engine's staged maps (dvp_download_maps_begin): the slot the view's new map is copied to on
	// the device, registered with Commit once it is there
	float* Reserve(int image_id, int w, int h) {
		Slot& s = maps_[image_id];
		if (s.w != w || s.h != h) {
			APD::UnsetResidentDepth(image_id);   // ... until Commit
			RankComm::DeviceFree(s.dev);
			s.dev = RankComm::DeviceAlloc((size_t)w * h);
			s.w = w;
			s.h = h;
		}
		return s.dev;
	}
	void Commit(int image_id) {
		const Slot& s = maps_[image_id];
		if (s.dev) APD::SetResidentDepth(image_id, s.dev, s.w, s.h);
	}
	void Release() {
		APD::ClearResidentDepths();
		for (auto& kv : maps_) RankComm::DeviceFree(kv.second.dev);
		maps_.clear();
	}
private:
	struct Slot { float* dev = nullptr; int w = 0, h = 0; };
	std::map<int, Slot> maps_;
};

// The float images of a pyramid level resident on the device: every image this rank's views use (as reference or as
// source) is uploaded ONCE per level; a view then takes its ten planes with device-to-device copies instead of the host
// re-sending 100 MB per image and per view that uses it (20 of the 50 ms of host time per full-resolution view).  Bounded
// by DVP_RESIDENT_IMAGES_GB (default 24): what does not fit keeps the host path.  Images whose size differs from the
// view's (padded / cropped sources) are simply not matched by APD::CudaSpaceInitialization.
class LevelImages {
public:
	~LevelImages() { Release(); }
	void Fill(const std::vector<Problem*>& owned, int scale) {
		Release();
		const char* e = std::getenv("DVP_RESIDENT_IMAGES_GB");
		const size_t budget = (size_t)(e ? std::max(0, std::atoi(e)) : 24) << 30;
		size_t used = 0;
		std::set<int> ids;
		for (const Problem* p : owned) { ids.insert(p->ref_image_id); ids.insert(p->src_image_ids.begin(), p->src_image_ids.end()); }
		if (owned.empty()) return;
		Problem q = *owned[0];
		q.scale_size = scale;
		for (int id : ids) {
			int oc = 0, orr = 0;
			const Mat img = APD::CachedImage(q, id, &oc, &orr);   // reference role: the image at its own size
			const size_t count = (size_t)img.cols * img.rows;
			if (img.empty() || used + count * 4 > budget) continue;
			float* dev = RankComm::DeviceAlloc(count);
			RankComm::HostToDevice(dev, img.ptr<float>(0), count);
			blocks_.push_back(dev);
			used += count * 4;
			APD::SetResidentImage(id, scale, dev, img.cols, img.rows, oc, orr);
		}
	}
	void Release() {
		APD::ClearResidentImages();
		for (float* b : blocks_) RankComm::DeviceFree(b);
		blocks_.clear();
	}
private:
	std::vector<float*> blocks_;
};

// The owner of a view (rank v % world) decodes + resizes its image at this level and broadcasts it; the others
// take it from the broadcast into their image cache: every image file is read by exactly one process and the
// decode work is spread over the ranks.
void ShareLevelImages(RankComm& comm, std::vector<Problem>& problems, const std::vector<int>& owner_of, int scale) {
	if (comm.world() <= 1) return;
	APD::ReserveImageCache(problems.size());
	for (Problem& p : problems) {
		p.scale_size = scale;
		const int owner = owner_of[(size_t)p.index];
		int meta[4] = { 0, 0, 0, 0 };   // cols, rows, original cols, original rows
		Mat img;
		if (comm.rank() == owner) {
			img = APD::CachedImage(p, p.ref_image_id, &meta[2], &meta[3]);
			meta[0] = img.cols;
			meta[1] = img.rows;
		}
		comm.BroadcastHost(meta, sizeof(meta), owner);
		if (comm.rank() != owner) img = Mat(meta[1], meta[0], CV_32FC1);
		comm.BroadcastHost(img.data, (size_t)meta[0] * meta[1] * sizeof(float), owner);
		if (comm.rank() != owner) APD::InsertCachedImage(p, p.ref_image_id, img, meta[2], meta[3]);
	}
}

// --images-on gpu: the owner of a view broadcasts the DECODED file once per job — meta, then 1 byte per pixel — and the others
// keep it in their decoded cache, from where every level of it is made on their device; no float image travels per level.
void ShareDecodedImages(RankComm& comm, const std::vector<Problem>& problems, const std::vector<int>& owner_of) {
	if (comm.world() <= 1) return;
	for (const Problem& p : problems) {
		const path file = p.dense_folder / "images" / (ToFormatIndex(p.ref_image_id) + ".jpg");
		const int owner = owner_of[(size_t)p.index];
		int meta[2] = { 0, 0 };   // cols, rows (0 x 0: the owner cannot read the file and will stop the job when it loads it)
		Mat gray;
		if (comm.rank() == owner) {
			gray = APD::DecodedGray(file);
			meta[0] = gray.cols;
			meta[1] = gray.rows;
		}
		comm.BroadcastHost(meta, sizeof(meta), owner);
		if (meta[0] <= 0 || meta[1] <= 0) continue;
		if (comm.rank() != owner) gray = Mat(meta[1], meta[0], CV_8UC1);
		comm.BroadcastHost(gray.data, (size_t)meta[0] * meta[1], owner);
		if (comm.rank() != owner) APD::InsertDecoded(file, gray);
	}
}

// apd --convert-from <colmap folder> <save folder> [options]: no engine context, no rank, no result store
int ConvertMain(int argc, char** argv) {
	const char* usage = "USAGE: apd --convert-from colmap_folder save_folder [--model-dir NAME] [--model-ext .txt|.bin] [--scale-factor F] [--max-d N] [--interval-scale F] [--sfm on|off] [--convert-on gpu|host] [--undistort on|off] [--gpu N]\n";
	if (argc < 4 || argv[2][0] == '-' || argv[3][0] == '-') { std::cerr << usage; return EXIT_FAILURE; }
	ConvertOptions o;
	o.colmap_folder = argv[2];
	o.save_folder = argv[3];
	for (int a = 4; a < argc; ++a) {
		const std::string s = argv[a];
		if (a + 1 >= argc) { std::cerr << s << " takes a value\n" << usage; return EXIT_FAILURE; }
		const std::string v = argv[++a];
		if (s == "--model-dir") o.model_dir = v;
		else if (s == "--model-ext") {
			if (v != ".txt" && v != ".bin") { std::cerr << "--model-ext takes .txt or .bin\n"; return EXIT_FAILURE; }
			o.model_ext = v;
		}
		else if (s == "--scale-factor") o.scale_factor = std::atof(v.c_str());
		else if (s == "--max-d") o.max_d = std::atoi(v.c_str());
		else if (s == "--interval-scale") o.interval_scale = std::atof(v.c_str());
		else if (s == "--sfm") {
			if (v != "on" && v != "off") { std::cerr << "--sfm takes on or off\n"; return EXIT_FAILURE; }
			o.sfm = v == "on";
		}
		else if (s == "--convert-on") {
			if (v != "gpu" && v != "host") { std::cerr << "--convert-on takes gpu or host\n"; return EXIT_FAILURE; }
			o.on_gpu = v == "gpu";
		}
		else if (s == "--undistort") {
			if (v != "on" && v != "off") { std::cerr << "--undistort takes on or off\n"; return EXIT_FAILURE; }
			o.undistort = v == "on";
		}
		else if (s == "--gpu") o.device = std::atoi(v.c_str());
		else { std::cerr << "unknown option " << s << "\n" << usage; return EXIT_FAILURE; }
	}
	std::error_code ec;
	std::filesystem::create_directories(o.save_folder, ec);
	std::string error;
	const auto t0 = std::chrono::steady_clock::now();
	if (!ConvertColmap(o, &error)) { std::cerr << "apd --convert-from: " << error << std::endl; return EXIT_FAILURE; }
	std::cout << "Converted " << o.colmap_folder.string() << " -> " << o.save_folder.string() << " (scores and resampling on the " << (o.on_gpu ? "device" : "host") << (o.undistort ? ", pictures undistorted" : "") << ", "
	          << std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() << " ms)" << std::endl;
	return EXIT_SUCCESS;
}

// apd --evaluate <recon.ply> --against <truth.ply> [options]: no engine context, no rank, no result store
int EvaluateMain(int argc, char** argv) {
	const char* usage = "USAGE: apd --evaluate recon.ply --against truth.ply | --against-scans FILE.mlp [--cube-size R] [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--evaluate-on gpu|host] [--gpu N] [--out FILE]\n"
	                    "       [--transform FILE] [--crop FILE] [--voxel-size S] [--save-prepared PREFIX]\n"
	                    "       [--refine-alignment V:D:N[,V:D:N...]] [--save-transform FILE]\n"
	                    "  --transform: 16 numbers (4 x 4, row-major) applied to the reconstruction; --crop: a SelectionPolygonVolume JSON, both clouds;\n"
	                    "  --voxel-size: both clouds down-sampled to one centroid per voxel of edge S; --save-prepared: <PREFIX>recon.ply and <PREFIX>truth.ply\n"
	                    "  --refine-alignment: ICP stages (voxel V, largest correspondence distance D, at most N steps) that refine the transform (the identity\n"
	                    "  without --transform) before the clouds are measured; Tanks and Temples' choice for a scene threshold t: t:80t:20,t/2:20t:20,t/2:2t:20;\n"
	                    "  --save-transform: the refined 4 x 4 matrix, a file --transform reads\n"
	                    "  --against-scans: the ground truth as the laser scans of a MeshLab project (ETH3D's scan_alignment.mlp); the accuracy then counts a point\n"
	                    "  away from the truth only where a scanner looked through it; --cube-size: texels along an edge of the scans' cube maps (a power of two,\n"
	                    "  16 ... 4096, default 1024)\n";
	if (argc < 3 || argv[2][0] == '-') { std::cerr << usage; return EXIT_FAILURE; }
	EvaluateOptions o;
	bool cube_given = false;
	o.recon = argv[2];
	for (int a = 3; a < argc; ++a) {
		const std::string s = argv[a];
		if (a + 1 >= argc) { std::cerr << s << " takes a value\n" << usage; return EXIT_FAILURE; }
		const std::string v = argv[++a];
		if (s == "--against") o.truth = v;
		else if (s == "--tolerances") {
			o.tolerances.clear();
			std::stringstream list(v);
			std::string item;
			while (std::getline(list, item, ',')) {
				char* end = nullptr;
				const float t = std::strtof(item.c_str(), &end);
				if (item.empty() || *end) { std::cerr << "--tolerances takes numbers separated by commas, got `" << item << "`\n"; return EXIT_FAILURE; }
				o.tolerances.push_back(t);
			}
			if (o.tolerances.empty() || o.tolerances.size() > 8) { std::cerr << "--tolerances takes 1 to 8 numbers\n"; return EXIT_FAILURE; }
		}
		else if (s == "--evaluate-on") {
			if (v != "gpu" && v != "host") { std::cerr << "--evaluate-on takes gpu or host\n"; return EXIT_FAILURE; }
			o.on_gpu = v == "gpu";
		}
		else if (s == "--gpu") o.device = std::atoi(v.c_str());
		else if (s == "--out") o.out = v;
		else if (s == "--transform") o.transform_file = v;
		else if (s == "--crop") o.crop_file = v;
		else if (s == "--voxel-size") {
			char* end = nullptr;
			o.voxel = std::strtod(v.c_str(), &end);
			if (v.empty() || *end || !(o.voxel > 0.0) || !std::isfinite(o.voxel)) { std::cerr << "--voxel-size takes a finite, positive number, got `" << v << "`\n"; return EXIT_FAILURE; }
		}
		else if (s == "--save-prepared") o.save_prepared = v;
		else if (s == "--refine-alignment") {
			std::string what;
			if (!ParseRefineStages(v, &o.refine, &what)) { std::cerr << what << "\n"; return EXIT_FAILURE; }
		}
		else if (s == "--save-transform") o.save_transform = v;
		else if (s == "--against-scans") o.truth_scans = v;
		else if (s == "--cube-size") {
			char* end = nullptr;
			const long R = std::strtol(v.c_str(), &end, 10);
			if (v.empty() || *end || R < 16 || R > 4096 || (R & (R - 1)) != 0) { std::cerr << "--cube-size takes a power of two, 16 ... 4096, got `" << v << "`\n"; return EXIT_FAILURE; }
			o.cube_size = (int)R;
			cube_given = true;
		}
		else { std::cerr << "unknown option " << s << "\n" << usage; return EXIT_FAILURE; }
	}
	if (!o.truth.empty() && !o.truth_scans.empty()) { std::cerr << "--against and --against-scans exclude each other\n" << usage; return EXIT_FAILURE; }
	if (o.truth.empty() && o.truth_scans.empty()) { std::cerr << "--against is required (or --against-scans)\n" << usage; return EXIT_FAILURE; }
	if (cube_given && o.truth_scans.empty()) { std::cerr << "--cube-size needs --against-scans\n" << usage; return EXIT_FAILURE; }
	std::string report, error;
	if (!EvaluateClouds(o, &report, &error)) { std::cerr << "apd --evaluate: " << error << std::endl; return EXIT_FAILURE; }
	std::cout << report << std::flush;
	return EXIT_SUCCESS;
}

// Everything that happens once per process before the view graph is used: the engine's defaults in the environment, the run's
// configuration, the process' place on the host, the rendezvous with the peers and the fatal hook.
std::unique_ptr<RankComm> SetUpProcess(const Options& opt, const std::vector<Problem>& problems) {
	std::filesystem::create_directories(opt.dense_folder / "APD");
	// The engine's sweep passes through a band of rows of at most 24 GB of cost records (the whole 25-Mpx view with 9 sources: 67 GB =
	// 2.3 s of fresh device memory, part of which the views running meanwhile wait for; 3 bands cost a geometric full-size pass 10 ms
	// per view in drained launches, 5 bands 20): a full-size context is 64 GB instead of 107.  Measured neutral on the ten-view
	// schedule (32.8 s either way).  DVP_SWEEP_BAND_GB in the environment wins; 0 = whole image.
	setenv("DVP_SWEEP_BAND_GB", "24", 0);
	// The strong update's plane cache (DVP_STRONG_REUSE) costs a full-size context 15.3 GB more (23.1 GB of records in place of the
	// 7.8 GB cost buffer): 4 contexts in flight are then 317 GB, more than the part has, and the contexts made last would lose
	// buffers they need more.  Off here unless the environment says otherwise (a driver with fewer views in flight may turn it on).
	setenv("DVP_STRONG_REUSE", "0", 0);
	// --strong-wide on: the three-launch strong update also for views with 17 ... 31 sources (a folder of the reference's converter
	// lists 20 per view), which otherwise take the monolithic kernel.  Same results.  DVP_STRONG_WIDE in the environment wins.
	if (opt.run.strong_wide) setenv("DVP_STRONG_WIDE", "1", 0);
	// The configuration is fixed before the decode threads start, so the plan's last index comes from the first image's header
	// (the plan proper follows PyramidLevels' decode of the same file; a file that does not decode runs no pass at all).
	RunConfig run = opt.run;
	int w = 0, h = 0;
	if (!problems.empty() && ImageFileSize(problems[0].dense_folder / "images" / (ToFormatIndex(problems[0].ref_image_id) + ".jpg"), &w, &h))
		run.final_iteration = (int)BuildPlan(LevelsOf(w, h), opt.min_scale, opt.geom_passes).size() - 1;
	SetRunConfig(run);
	dvp_jpeg_set_entropy(run.entropy_on_device ? 1 : 0);   // (before the decode threads start)
	SetHostThreadShare(opt.world);
	if (opt.world > 1) std::cout << "rank " << opt.rank << " of " << opt.world << ": " << HostThreads() << " host threads (of " << std::thread::hardware_concurrency() << " cores)" << std::endl;
	APD::SetDevice(opt.gpu);
	{   // before any thread is started and any large block is touched
		const int node = RankComm::BindProcessNearDevice(opt.gpu);
		if (node >= 0) std::cout << "GPU " << opt.gpu << " hangs off NUMA node " << node << ": process confined to its CPUs" << std::endl;
	}
	APD::SetSeed(opt.seed);
	SetResultCache(!opt.sync_io);
	std::unique_ptr<RankComm> comm(new RankComm(opt.rank, opt.world, opt.gpu, (opt.dense_folder / "APD" / ".rccl_id").string(), opt.job, opt.collective_timeout_s, opt.transport));
	// every print-and-exit of the host library (unreadable image, missing weak.bin, engine error ...) becomes an agreed
	// abort of the whole job when there are peers
	DvpSetFatalHook([](const char* msg) { if (RankComm* c = RankComm::Current()) if (c->world() > 1) c->Abort(msg); });
	return comm;
}

// this rank's images are decoded in the background from now on (every pyramid level is made from the decoded file)
void PrefetchOwnImages(const Options& opt, const std::vector<Problem>& problems, const std::vector<int>& owner_of) {
	std::vector<path> mine;
	for (const Problem& p : problems)
		if (owner_of[(size_t)p.index] == opt.rank) mine.push_back(opt.dense_folder / "images" / (ToFormatIndex(p.ref_image_id) + ".jpg"));
	if (opt.world == 1)   // a single rank also reads every source image itself
		for (const Problem& p : problems)
			for (int id : p.src_image_ids) mine.push_back(opt.dense_folder / "images" / (ToFormatIndex(id) + ".jpg"));
	APD::PrefetchDecoded(mine);
}

// what the passes of a run share
struct Job {
	const Options& opt;
	RankComm& comm;
	std::vector<Problem>& problems;
	const std::vector<int>& owner_of;
	const std::vector<Pass>& plan;
	const int round_num;
	Lap& lap;   // DVP_HOST_TIMING: what the driver does between the passes
	std::unique_ptr<DepthExchange> exchange;   // --jacobi / several ranks: a pass reads the previous pass' maps
	std::unique_ptr<InPlaceDepths> inplace;    // else, unless --sync-io: a view reads the maps its predecessors made in the same pass
	LevelImages level_images;
	int shared_scale = -1;
};

// The edge / label maps of an A pass (main.cpp:480: GetProblemEdges before every view).  Round 4 made the NEXT view's maps
// while the GPU worked on the current one — on the one background worker, behind that view's clean-up job: at the coarse
// levels a view's kernels take 20-70 ms, its label map (Roberts cross + components + Hough lines on the FULL-size image)
// longer, and SupportInitialization waited 32 of 59 ms per view (profiles/r04g_e2e_apd.txt, pass 0).  Now every owned
// view's maps are announced at the start of the pass and made by a few helper threads in view order; a view only waits
// if its own maps are not there yet (LoadResult waits for announced files).  Same files (store.cpp).
std::vector<std::future<void>> StartEdgeJobs(const Job& d, size_t it, const std::vector<Problem*>& owned) {
	const Pass& pass = d.plan[it];
	std::vector<Problem> views;
	if (pass.geom_index < 0)
		for (const Problem* p : owned) views.push_back(*p);
	// ... and during the last pass of a level, the maps of the NEXT level's A pass (its first view used to wait for its
	// own label map: 0.6 s at full size)
	if (it + 1 < d.plan.size() && d.plan[it + 1].scale != pass.scale && d.plan[it + 1].geom_index < 0)
		for (const Problem* p : owned) {
			Problem q = *p;
			ConfigurePass(q, d.plan[it + 1], (int)it + 1, d.opt.iters, d.round_num);
			views.push_back(q);
		}
	struct Queue { std::mutex m; size_t next = 0; std::vector<std::pair<Problem, std::vector<path>>> items; };
	auto q = std::make_shared<Queue>();
	for (const Problem& p : views) {
		std::vector<path> outs = ProblemEdgeOutputs(p);   // (what exists or is announced already is not made again)
		for (const path& f : outs) ExpectResult(f);
		if (!outs.empty()) q->items.emplace_back(p, std::move(outs));
	}
	std::vector<std::future<void>> jobs;
	const int helpers = (int)std::min<size_t>(q->items.size(), (size_t)std::max(1, std::min(4, HostThreads() / 4)));
	for (int h = 0; h < helpers; ++h)
		jobs.push_back(std::async(std::launch::async, [q]() {
			// two threads per helper: with full-size teams the helpers starved the thread that issues the launches — the GPU
			// idled between kernels (RunPatchMatch of a 1552x1032 view: 67 -> 131 ms)
			SetThisThreadHostThreads(2);
			for (;;) {
				size_t i;
				{ std::lock_guard<std::mutex> lk(q->m); i = q->next++; }
				if (i >= q->items.size()) return;
				GetProblemEdges(q->items[i].first, q->items[i].second);
			}
		}));
	return jobs;
}

// Views in flight.  The reference visits the views of a pass one after the other (main.cpp:479-486) and a view of a
// geometric pass reads the maps the views before it have just written — that order is kept.  Where no view reads another
// view's result of the SAME pass — a photometric pass, or any pass with the depth exchange (--jacobi / several ranks: maps of
// the previous pass) — and the level is small, two or more views run at once, each on its own engine context and stream:
// a 776x516 view is 6 k waves for a 256-CU part and 20 ms of kernels between 10 ms of host work (profiles/r04g_e2e_apd.txt).
// Same files either way (every view's inputs are fixed before the pass).
int ViewsInFlight(const Job& d, const Pass& pass, const std::vector<Problem*>& owned) {
	if (d.opt.sync_io || !(pass.geom_index < 0 || d.exchange) || owned.empty()) return 1;
	int in_flight = 1, lw = 0, lh = 0;
	if (APD::LevelSize(*owned[0], pass.scale, &lw, &lh) && (size_t)lw * lh <= (size_t)d.opt.in_flight_pixels) in_flight = d.opt.views_in_flight > 0 ? d.opt.views_in_flight : 2;
	return (int)std::min<size_t>((size_t)std::max(1, in_flight), owned.size());
}

// One owned view of a pass, and its new depth map recorded: in `mine` for the exchange, or in the in-place maps — on the device
// already when the view staged its maps there (Reserve ... Commit), else uploaded (Update).  `results`: the lock the worker
// threads of a pass share (null on the serial path) around `mine`, the in-place maps and the order of the views' log blocks;
// a worker's view logs into a buffer that is printed in one piece.
void RunOwnedView(Job& d, Problem& problem, std::map<int, Mat>& mine, std::mutex* results) {
	std::ostringstream log;
	if (results) SetViewLog(&log);
	bool on_device = false;
	ViewResult r = ProcessProblem(problem, [&](int w, int h) -> float* {
		if (!d.inplace || !Run().device_maps) return nullptr;
		std::unique_lock<std::mutex> lk;
		if (results) lk = std::unique_lock<std::mutex>(*results);
		on_device = true;
		return d.inplace->Reserve(problem.ref_image_id, w, h);
	});
	std::unique_lock<std::mutex> lk;
	if (results) {
		SetViewLog(nullptr);
		lk = std::unique_lock<std::mutex>(*results);
		std::cout << log.str() << std::flush;
	}
	if (d.exchange) mine[problem.index] = r.depth;
	if (d.inplace && on_device) d.inplace->Commit(problem.ref_image_id);
	else if (d.inplace) d.inplace->Update(problem.ref_image_id, r.depth);
}

// last pass of a level: the next level's context and float images are made by helper threads while the GPU works
void PrepareNextLevel(const Job& d, const Pass& next, const std::vector<Problem*>& owned) {
	int nw = 0, nh = 0;
	if (APD::LevelSize(*owned[0], next.scale, &nw, &nh)) APD::PrewarmContext(nw, nh, (int)owned[0]->src_image_ids.size() + 1, next.scale);
	std::vector<Problem> mine_next;
	for (const Problem* p : owned) mine_next.push_back(*p);
	if (!d.opt.run.images_on_device) APD::PrefetchLevelImages(mine_next, next.scale);
}

void RunPass(Job& d, size_t it) {
	const Options& opt = d.opt;
	const Pass& pass = d.plan[it];
	const bool new_level = pass.scale != d.shared_scale;
	d.lap.t = std::chrono::steady_clock::now();
	if (new_level) {
		if (!opt.run.images_on_device) ShareLevelImages(d.comm, d.problems, d.owner_of, pass.scale);
		d.shared_scale = pass.scale;
		if (d.exchange) d.exchange->Release();   // maps of the coarser level do not fit this one (and its A pass has no geometric term)
	}
	std::map<int, Mat> mine;
	std::vector<Problem*> owned;
	for (Problem& problem : d.problems) {
		ConfigurePass(problem, pass, (int)it, opt.iters, d.round_num);
		if (d.owner_of[(size_t)problem.index] == opt.rank) owned.push_back(&problem);
	}
	if (new_level && !opt.sync_io && !opt.run.images_on_device) d.level_images.Fill(owned, pass.scale);   // (--images-on gpu: the views make their levels from the store)
	if (new_level) d.lap("level " + std::to_string(pass.level) + ": images shared + resident on the device");
	if (!opt.sync_io && it + 1 < d.plan.size() && d.plan[it + 1].scale != pass.scale && !owned.empty()) PrepareNextLevel(d, d.plan[it + 1], owned);
	std::vector<std::future<void>> edge_jobs;
	if (!opt.sync_io) edge_jobs = StartEdgeJobs(d, it, owned);
	const int in_flight = ViewsInFlight(d, pass, owned);
	// the fusion's colour images are decoded while the last pass runs (rank 0 fuses)
	if (it + 1 == d.plan.size() && opt.fusion && opt.rank == 0 && !opt.sync_io) PrefetchFusionImages(opt.dense_folder, d.problems);
	d.lap("pass " + std::to_string(it) + ": helpers started");
	const auto pass_t0 = std::chrono::steady_clock::now();
	if (in_flight <= 1) {
		for (Problem* problem : owned) {
			if (pass.geom_index < 0 && opt.sync_io) GetProblemEdges(*problem);   // main.cpp:480, synchronously
			RunOwnedView(d, *problem, mine, nullptr);
		}
	} else {
		std::atomic<size_t> next{0};
		std::mutex results;
		std::vector<std::thread> workers;
		const int team = std::max(2, HostThreads() / in_flight);
		for (int wkr = 0; wkr < in_flight; ++wkr)
			workers.emplace_back([&, team]() {
				RankComm::BindThisThread(opt.gpu);   // HIP's current device is per thread
				SetThisThreadHostThreads(team);
				for (size_t k = next++; k < owned.size(); k = next++) RunOwnedView(d, *owned[k], mine, &results);
			});
		for (std::thread& t : workers) t.join();
	}
	if (HostTiming()) {   // (one write: the background jobs of the pass' views may still be printing their own timing lines)
		std::ostringstream line;
		line << "Pass " << it << ": " << owned.size() << " views in " << std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - pass_t0).count() / 1000.0
		     << " ms, " << in_flight << " in flight\n";
		std::cout << line.str() << std::flush;
	}
	// With peers, a view whose size differs from a source's takes that source's depth map from APD/<id>/depths.dmb
	// (APD.cpp fallback from the resident maps to LoadResult): the owner's background writer must have put this
	// pass' files on disk BEFORE the barrier lets anyone into the next pass, or the reader sees the previous pass'
	// map (or none) depending on timing.  One rank has no other reader: its cache serves its own next pass.
	d.lap.t = std::chrono::steady_clock::now();
	for (auto& j : edge_jobs) j.get();
	if (opt.world > 1) FlushResults();
	if (d.exchange) WaitBackgroundJobs();      // (the maps of `mine` are filled by the views' background jobs)
	if (d.exchange) d.exchange->Publish(mine);   // collective: also the barrier between passes
	else d.comm.Barrier();
	d.lap("pass " + std::to_string(it) + ": helpers joined, exchange / barrier");
	if (pass.geom_index == opt.geom_passes - 1 || (opt.geom_passes == 0 && pass.geom_index < 0)) std::cout << "Round: " << pass.level << " done\n";
}

}  // namespace

int main(int argc, char** argv) {
	if (argc >= 2 && std::string(argv[1]) == "--convert-from") return ConvertMain(argc, argv);
	if (argc >= 2 && std::string(argv[1]) == "--evaluate") return EvaluateMain(argc, argv);
	if (argc < 2) { std::cerr << kApdUsage; return EXIT_FAILURE; }
	const Options opt = ParseOptions(argc, argv);
	Lap lap{ "[main] " };
	std::vector<Problem> problems = ReadViewGraph(opt.dense_folder, opt.max_src);   // (read first: the set-up sizes the plan from the first view's image)
	for (Problem& p : problems) p.show_medium_result = opt.previews;
	const std::unique_ptr<RankComm> comm = SetUpProcess(opt, problems);
	std::cout << "There are " << problems.size() << " problems needed to be processed!" << std::endl;
	const std::vector<int> owner_of = AssignViews(problems, opt.world);
	if (opt.world > 1) {
		std::cout << "rank " << opt.rank << " owns views";
		for (const Problem& p : problems) if (owner_of[(size_t)p.index] == opt.rank) std::cout << " " << p.index;
		std::cout << std::endl;
	}
	PrefetchOwnImages(opt, problems, owner_of);
	lap("start-up (options, rendezvous, view graph, decode prefetch started)");
	const int round_num = PyramidLevels(problems);
	lap("PyramidLevels (first image decoded)");
	std::cout << "Round nums: " << round_num << std::endl;
	const std::vector<Pass> plan = BuildPlan(round_num, opt.min_scale, opt.geom_passes);
	Job d{ opt, *comm, problems, owner_of, plan, round_num, lap };
	if (opt.jacobi) { d.exchange.reset(new DepthExchange(*comm, problems, owner_of)); APD::SetResidentDownloader(&RankComm::DeviceToHost); }
	else if (!opt.sync_io) d.inplace.reset(new InPlaceDepths());
	if (opt.run.images_on_device) {
		ShareDecodedImages(*comm, problems, owner_of);
		lap("decoded images shared");
	}
	for (size_t it = 0; it < plan.size(); ++it) RunPass(d, it);
	if (opt.run.images_on_device && HostTiming()) std::cout << "[main] decoded images on the device: " << APD::StoredImageBytes() << " bytes" << std::endl;
	lap.t = std::chrono::steady_clock::now();
	if (d.exchange) d.exchange->Release();
	d.exchange.reset();
	d.inplace.reset();
	d.level_images.Release();
	APD::ReleasePooledContext();
	lap("contexts and resident maps released");
	// Several ranks: every result file of this rank is on disk before rank 0's fusion reads the folder.  One rank: the fusion takes
	// the maps from the result cache (LoadResult waits for a map whose background job has not published it yet), so the last views'
	// files are written while it runs; ShutdownResultStore waits for them.
	if (opt.world > 1 || opt.sync_io) FlushResults();
	lap("FlushResults (background jobs + file writes)");
	comm->Barrier();
	if (opt.fusion && opt.rank == 0) {
		SetFusionOnHost(opt.fusion_on_host);   // all three variants run on the GPU (dvp_fuse_*) unless --fusion-on host
		SetFusionDevice(opt.gpu);
		if (opt.fusion_kind == "tat-intermediate") RunFusion_TAT_Intermediate(opt.dense_folder, problems);
		else if (opt.fusion_kind == "tat-advanced") RunFusion_TAT_advanced(opt.dense_folder, problems);
		else RunFusion(opt.dense_folder, problems);
	}
	ShutdownResultStore();
	lap("fusion + shutdown");
	std::cout << "All done\n";
	return EXIT_SUCCESS;
}
