// dvp_forms.hpp — which form every launch site of RunPatchMatch takes.  The DVP_* switches are parsed into FormSwitches; pure
// functions turn them, with the facts of a launch and whether a form's optional buffers fit (`*_fits`: a run-time result of the
// context), into the kernels to issue.  The engine reads the switches when a context is created, the host emulation (tests/emul)
// at every launch; tests/test_forms.py holds the rule as a table.  Plain C++: no HIP, no device types.
#ifndef DVP_FORMS_HPP_
#define DVP_FORMS_HPP_

#include "../../include/dvp_mvs.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace dvp {

constexpr int kNarrowViews = 8;   // view capacity of the narrow strong-update instantiation
constexpr int kGrp = 4, kGrpWide = 2;   // WEAK pixels per wave of the phased weak update's evaluation launches at most (kGrpWide: E0)
#ifndef DVP_SWEEP_ROWS
#define DVP_SWEEP_ROWS 14
#endif
constexpr int kSweepRows = DVP_SWEEP_ROWS;   // rows of a dvp_sweep_eval tile (64 x kSweepRows pixels; 14: patch table 18 KB + list 1.75 KB + two cameras = 20 KB, 8 workgroups per CU)
constexpr int kSweepFields = 73;    // [0, 61): slot pd + 30 — ncc for |pd| <= 5, ncc + factor * geom otherwise; [61, 72): geom of slot |pd| <= 5
constexpr int sweep_window(const DvpParams& P) { int cw = P.weak_peak_radius + 1; if (cw < 5) cw = 5; if (cw > 30) cw = 30; return cw; }
constexpr size_t sweep_cost_floats(size_t L, int S) { return ((L + 63) / 64) * 64 * (size_t)S * kSweepFields; }
// Is sweep slot pd (-30 ... 30, line entry pd + 30) evaluated, fetched and folded under a window of half-width cw (sweep_window)?
// No decision reads the two end slots: the peak searches of DepthToWeak are `for (i = 2; i < 59; ++i)` over the entries i - 1, i,
// i + 1, i.e. 1 ... 59.  Entry 60 is read nowhere else.  Entry 0 is read once more, as p_costs[min_peak] with min_peak == 0, i.e. when
// the line has no peak below 2 — and that statement is reached only by pixels with a central peak <= 0.5 (depth_to_weak_px:
// `if (!central_peak) state = DVP_WEAK` comes first; sweep_decide2_cw returns unless SWF_PEAK is set), whose entries i - 1, i, i + 1
// lie inside 1 ... 59 and make the same i a peak of the full search, so min_peak != 0 there.  LocalRefine reads the slots -5 ... 5.
// So both are left out and their line entries are the constant 2, the value of a slot outside the depth range.
// cw == 30 (weak_peak_radius >= 29, the whole line in the first stage): the argument holds there too (the central-peak test skips
// i < 2 and i > 58), but the slots stay: in dvp_sweep_eval they would have to be stepped over in the middle of the first stage's
// walk, and the evaluator's schedule pays for every live value in that loop (profiles/sweep_dead_slots.txt).
// all_slots: DVP_SWEEP_ALL_SLOTS=1, all 61 everywhere (A/B).
constexpr bool sweep_slot_read(int cw, int pd, bool all_slots) { return all_slots || cw == 30 || (pd > -30 && pd < 30); }

inline bool env_flag(const char* name, bool unset) { const char* e = getenv(name); return e ? atoi(e) != 0 : unset; }

struct FormSwitches {   // unset defaults; =0 / =1 are atoi(e) != 0, "(present)" variables count by being set
	bool no_images8 = false, no_images16 = false;   // DVP_NO_IMAGES8 / _16 (present): such sets keep the float planes (A/B measurements)
	bool strong_split = true, strong_reuse = true;  // DVP_STRONG_SPLIT=0: the monolithic kernel; DVP_STRONG_REUSE=0: no plane cache
	bool refine_lanes = true, eval_items = true;    // DVP_REFINE_LANES=0: dvp_strong_refine; DVP_EVAL_ITEMS=0: dvp_strong_eval (a pixel per lane)
	int strong_wide = 0;          // DVP_STRONG_WIDE=1: the split form also for 17 <= S <= 31 (dvp_strong_decide_wide); =2: that decision kernel at every S (A/B)
	bool sweep_split = true, sweep_force = false;   // DVP_SWEEP_SPLIT=0: the fused per-pixel kernel; =2: the passes also without the geometric term
	bool sweep_all_slots = false; // DVP_SWEEP_ALL_SLOTS=1: the sweep site also evaluates the two end slots no decision reads (sweep_slot_read; A/B)
	double sweep_band_gb = 0.0;   // DVP_SWEEP_BAND_GB=g: sweep_cost holds a band of rows of at most g GB (0: the whole image)
	bool sweep_list = true;       // DVP_SWEEP_LIST=0: the passes' evaluation launches walk tiles (dvp_sweep_eval) instead of per-view lists (sweep_eval_form; A/B)
	bool anchor_tab_off = false;  // DVP_WEAK_ANCHOR_TAB=0: the weak update forms the reference side per item
	bool gn_wave = false, ransac_wave = false;      // DVP_GN_WAVE=1 / DVP_RANSAC_WAVE=1: a wave per WEAK pixel (measured no faster)
	int cand_mask_mode = -1;      // DVP_CAND_MASK=1 / 0 forces masked / full candidates
	bool weak_phased = true, weak_split_colours = false;   // DVP_WEAK_PHASED=0: the one-wave kernel; DVP_WEAK_SPLIT_COLOURS (present): two launch sites
	int weak_phased_min = 8192;   // DVP_WEAK_PHASED_MIN: WEAK pixels of a launch below which the one-wave kernel is used (<= 0: never)
	int weak_run[4] = { 64, 256, 1024, 1024 }, weak_group[4] = { 1, 4, 4, 2 };   // DVP_WEAK_RUNS / _GROUPS=a,b,c,d: WEAK pixels per XCD run / per wave of E0 / E1 / E2a / E2b
};
inline FormSwitches read_form_switches() {
	FormSwitches s;
	s.no_images8 = getenv("DVP_NO_IMAGES8") != nullptr;
	s.no_images16 = getenv("DVP_NO_IMAGES16") != nullptr;
	s.strong_split = env_flag("DVP_STRONG_SPLIT", true);
	s.strong_reuse = env_flag("DVP_STRONG_REUSE", true);
	s.refine_lanes = env_flag("DVP_REFINE_LANES", true);
	s.eval_items = env_flag("DVP_EVAL_ITEMS", true);
	if (const char* e = getenv("DVP_STRONG_WIDE")) { const int v = atoi(e); s.strong_wide = v == 0 ? 0 : (v == 2 ? 2 : 1); }
	if (const char* e = getenv("DVP_SWEEP_SPLIT")) { s.sweep_split = atoi(e) != 0; s.sweep_force = atoi(e) == 2; }
	s.sweep_all_slots = env_flag("DVP_SWEEP_ALL_SLOTS", false);
	if (const char* e = getenv("DVP_SWEEP_BAND_GB")) s.sweep_band_gb = atof(e);
	s.sweep_list = env_flag("DVP_SWEEP_LIST", true);
	s.anchor_tab_off = !env_flag("DVP_WEAK_ANCHOR_TAB", true);
	s.gn_wave = env_flag("DVP_GN_WAVE", false);
	s.ransac_wave = env_flag("DVP_RANSAC_WAVE", false);
	if (const char* e = getenv("DVP_CAND_MASK")) s.cand_mask_mode = atoi(e) != 0 ? 1 : 0;
	s.weak_phased = env_flag("DVP_WEAK_PHASED", true);
	if (const char* e = getenv("DVP_WEAK_PHASED_MIN")) s.weak_phased_min = atoi(e);
	int g[4];
	if (const char* e = getenv("DVP_WEAK_RUNS"))
		if (sscanf(e, "%d,%d,%d,%d", &g[0], &g[1], &g[2], &g[3]) == 4)
			for (int i = 0; i < 4; ++i) s.weak_run[i] = g[i] < 1 ? 1 : g[i];
	if (const char* e = getenv("DVP_WEAK_GROUPS"))
		if (sscanf(e, "%d,%d,%d,%d", &g[0], &g[1], &g[2], &g[3]) == 4)
			for (int i = 0; i < 4; ++i) s.weak_group[i] = g[i] < 1 ? 1 : (g[i] > kGrp ? kGrp : g[i]);   // (E0: at most kGrpWide, applied by weak_form)
	s.weak_split_colours = getenv("DVP_WEAK_SPLIT_COLOURS") != nullptr;
	return s;
}

// The image set's format: 0 float row pairs, 1 byte tiles, 2 binary16 tiles.  `inexact`: tile_pair_rule's bits over every texel.
inline int image_format(const FormSwitches& s, unsigned inexact) {
	return (inexact == 0 && !s.no_images8) ? 1 : ((inexact == 1 && !s.no_images8 && !s.no_images16) ? 2 : 0);
}

// Strong update: three launches (evaluate / decide / refine) for S <= 16 — with DVP_STRONG_WIDE for S <= 31 — or one monolithic kernel.
enum StrongKernel { STRONG_SPLIT, STRONG_MONO_V8, STRONG_MONO_V16, STRONG_MONO };
struct StrongForm {
	StrongKernel kernel;
	bool eval_items;     // split: dvp_strong_eval_items, else dvp_strong_eval
	int decide;          // split: the view bracket of dvp_strong_decide_v{4,6,8,10,12,16}; 32: dvp_strong_decide_wide (any S <= 31, the vectors streamed)
	bool refine_lanes;   // split: dvp_strong_refine_lanes, else dvp_strong_refine
	bool plan;           // dvp_strong_plan runs after the sample search (the plane cache exists)
};
// image_set_bytes: all row-pair planes — dvp_strong_refine_lanes addresses them with 32-bit byte offsets
inline StrongForm strong_form(const FormSwitches& s, int S, bool split_fits, bool have_reuse_hdr, unsigned long long image_set_bytes) {
	const bool wide = s.strong_wide != 0 && S > 16 && S <= 31;
	if (!(s.strong_split && split_fits && (S <= 16 || wide))) return { S <= kNarrowViews ? STRONG_MONO_V8 : (S <= 16 ? STRONG_MONO_V16 : STRONG_MONO), false, 0, false, false };
	const int bracket = (wide || s.strong_wide == 2) ? 32 : (S <= 4 ? 4 : S <= 6 ? 6 : S <= 8 ? 8 : S <= 10 ? 10 : S <= 12 ? 12 : 16);
	return { STRONG_SPLIT, s.eval_items, bracket, s.refine_lanes && image_set_bytes < (1ull << 32), have_reuse_hdr };
}

// Weak update: eight launches over the WEAK list (dvp_weak_phased.hpp) or one wave per WEAK pixel, with or without the anchor table.
// (A few thousand WEAK pixels fill the machine in no form: the eight launches cost 4.4 against 1.7 ms at 3104x2064 with 0.2 % WEAK.)
enum WeakKernel { WEAK_PHASED, WEAK_WAVE, WEAK_WAVE_NOTAB };
struct WeakForm {
	WeakKernel kernel;
	int group[4], run[4];   // phased: WEAK pixels per wave and per XCD run of E0 / E1 / E2a / E2b
};
inline WeakForm weak_form(const FormSwitches& s, bool table_present, bool phase_fits, int count) {
	WeakForm f{};
	const bool phased = s.weak_phased && phase_fits && (count >= s.weak_phased_min || s.weak_phased_min <= 0);
	f.kernel = !table_present ? WEAK_WAVE_NOTAB : (phased ? WEAK_PHASED : WEAK_WAVE);
	for (int i = 0; i < 4; ++i) {
		const int cap = i == 0 ? kGrpWide : kGrp;
		f.group[i] = s.weak_group[i] < cap ? s.weak_group[i] : cap;
		f.run[i] = s.weak_run[i];
	}
	return f;
}
// dvp_run_patchmatch issues both colours of a weak update as one launch site
inline bool weak_joins_colours(const FormSwitches& s, bool table_fits, bool phase_fits) {
	return s.weak_phased && phase_fits && !s.anchor_tab_off && table_fits && !s.weak_split_colours;
}

// DepthToWeak (+ LocalRefine when `fused`: dvp_run_patchmatch's one launch site for both).  The passes pay where the geometric term
// rides along (cfg3: 622 -> 536 ms); without it (cfg2) they measure 63 ms against the fused kernel's 59: DVP_SWEEP_SPLIT=2 forces them.
enum SweepKernel { SWEEP_PASSES, SWEEP_FUSED, SWEEP_SEPARATE };
struct SweepForm {
	SweepKernel kernel;
	bool second_eval;     // passes: the rest of the line is evaluated too (the central window leaves slots over)
	bool border_kernel;   // passes: dvp_sweep_border takes the 6-pixel frame; false: the fused kernel does, border pixels only
};
inline SweepForm sweep_form(const FormSwitches& s, bool fused, const DvpParams& P, bool sweep_fits, int W, int H) {
	if (fused && s.sweep_split && sweep_fits && (P.geom_consistency || s.sweep_force)) return { SWEEP_PASSES, sweep_window(P) < 30, W >= 12 && H >= 12 };
	return { fused ? SWEEP_FUSED : SWEEP_SEPARATE, false, false };
}
// The evaluation launches of the passes: from per-view (pixel, view) lists, a wave = consecutive rounds of one view's list
// (dvp_sweep_eval_list, dvp_sweep_list.hpp), or tile by tile with the list of a tile in LDS (dvp_sweep_eval).  Same evaluations, same
// bits; the lists leave only the last round of a view part-empty instead of the last round of every (tile, view).
// list_fits: the list buffers could be had (dvp_ctx::sweep_list_fits).
enum SweepEval { SWEEP_EVAL_TILES, SWEEP_EVAL_LISTS };
inline SweepEval sweep_eval_form(const FormSwitches& s, const SweepForm& f, bool list_fits) {
	return (f.kernel == SWEEP_PASSES && s.sweep_list && list_fits) ? SWEEP_EVAL_LISTS : SWEEP_EVAL_TILES;
}
// rows of a band of the passes' cost buffer (a multiple of the evaluation tile's rows); 0 = the whole image
inline int sweep_band_rows(const FormSwitches& s, int W, int H, int S) {
	if (!(s.sweep_band_gb > 0.0)) return 0;
	const int bands = (int)std::ceil((double)sweep_cost_floats((size_t)W * H, S) * sizeof(float) / (s.sweep_band_gb * 1e9));
	if (bands <= 1) return 0;
	const int rows = ((H + bands - 1) / bands + kSweepRows - 1) / kSweepRows * kSweepRows;
	return rows < H ? rows : 0;
}

// Visibility-prior candidates of dvp_run_patchmatch: at anchor pixels only (below 4 % WEAK: dvp_ctx::cand_mask), or at every pixel.
inline bool candidates_masked(const FormSwitches& s, int weak_count, size_t L, bool mask_fits) {
	return weak_count > 0 && mask_fits && (s.cand_mask_mode == 1 || (s.cand_mask_mode < 0 && (size_t)weak_count * 25 < L));
}

}  // namespace dvp
#endif
