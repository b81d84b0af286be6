// driver.h — what `apd <dense_folder>` is told and the schedule it derives from it: the command line and the pass list (driver.cpp)
#ifndef DVP_HOST_DRIVER_H_
#define DVP_HOST_DRIVER_H_
#include "APD.h"

extern const char* const kApdUsage;   // the one usage text of `apd <dense_folder>`
extern const char* const kApdEntropyUsage;   // ... and what `--entropy-on gpu` without `--decode-on gpu` is refused with

struct Options {
	path dense_folder;
	int gpu = 0, max_src = 0, iters = 3, min_scale = 2, geom_passes = 3, rank = 0, world = 1;
	uint64_t seed = 1234;
	bool fusion = true, jacobi = false;
	int collective_timeout_s = 600;
	bool sync_io = false;                  // --sync-io: no result cache / background worker / device rescale: the reference's synchronous file flow
	bool host_rescale = false;             // --host-rescale: the coarser level's maps are up-sampled on the host
	RunConfig run;                         // --labels, the six --X-on host|gpu, --strong-wide on|off; device_rescale and device_maps follow from the two above
	bool previews = false;                 // --previews: the reference's show_medium_result preview images (depth/normal/weak_<it>.jpg, weak.png, rawedge_<s>.jpg)
	int views_in_flight = 0;               // --views-in-flight N: that many views of a pass at once (default 2) where the order allows it and the level is small; 1 = never
	long long in_flight_pixels = 2 << 20;  // ... "small" = at most this many pixels (--in-flight-pixels)
	std::string job, transport = "rccl";
	bool fusion_on_host = false;           // --fusion-on host: RunFusion on the host's cores instead of the GPU (same .ply)
	std::string fusion_kind = "eth";   // eth | tat-intermediate | tat-advanced (APD.h:52-54; the reference's main calls the first)
};
// argv as main got it (argv[1] = the dense folder).  Unknown options are ignored and a value option at the end of the line
// reads as 0; a word that a choice option does not take ends the process with "--X takes A or B".
Options ParseOptions(int argc, char** argv);

// one pass of the schedule
struct Pass {
	int level;        // pyramid level (0 = coarsest)
	int scale;        // down-sampling factor of that level
	int geom_index;   // -1: the A pass, else the REFINE_ITER pass number
};
// the pass list: level i has scale 2^(round_num-1-i); levels run while the scale is >= min_scale
// (min_scale = 2 reproduces `i < round_num - 1`, main.cpp:450; a single-level pyramid always runs)
std::vector<Pass> BuildPlan(int round_num, int min_scale, int geom_passes);
void ConfigurePass(Problem& problem, const Pass& pass, int iteration, int iters, int round_num);   // main.cpp:457-478, 488-502
#endif
