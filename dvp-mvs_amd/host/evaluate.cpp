// evaluate.cpp — `apd --evaluate recon.ply --against truth.ply` (evaluate.h): both clouds read, prepared when --transform, --crop or
// --voxel-size ask for it (csrc/dvp_cloudprep.hpp), the two directions counted on the device (dvp_cloud_evaluate, or
// dvp_cloud_evaluate_prepared) or by the same text on the host (csrc/dvp_cloudeval.hpp: the double loop up to 2^24 pairs, the grid
// walked serially above), and the report, whose figures come from the integer counts alone.  --refine-alignment first refines the
// reconstruction's matrix by ICP stages (csrc/dvp_cloudicp.hpp: dvp_cloud_refine_alignment, or the same text on the host), and the
// evaluation takes the refined matrix as if --transform had given it.  --against-scans takes the ground truth as the laser scans of a
// MeshLab project (csrc/dvp_cloudscan.hpp: dvp_cloud_evaluate_scans, or the same text on the host): their points brought into the scene
// are the truth cloud, and the accuracy column becomes the observed-space one.
#include "evaluate.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <new>
#include <sstream>

#include "../../include/dvp_mvs.h"
#include "../csrc/dvp_cloudeval.hpp"
#include "../csrc/dvp_cloudicp.hpp"
#include "../csrc/dvp_cloudscan.hpp"

std::string EvaluateReport(const EvaluateOptions& o, const long long num[2], const long long used[2], const long long* within_recon, const long long* within_truth,
                           const long long* counts, const std::string& scan_lines, const long long* free_space) {
	char text[256];
	// every point dropped for a non-finite coordinate: as read, after the transform, or after the rounding of a prepared point to binary32
	const long long skipped[2] = { counts ? (num[0] - counts[1]) + (counts[3] - used[0]) : num[0] - used[0], counts ? (num[1] - counts[5]) + (counts[7] - used[1]) : num[1] - used[1] };
	std::string report = "reconstruction " + o.recon + " " + std::to_string(used[0]) + " points (" + std::to_string(skipped[0]) + " skipped)\n" +
	                     "ground_truth " + o.truth + " " + std::to_string(used[1]) + " points (" + std::to_string(skipped[1]) + " skipped)\n" + scan_lines;
	for (int c = 0; c < 2 && counts; ++c)
		report += std::string("prepared ") + (c == 0 ? "reconstruction: " : "ground_truth: ") + std::to_string(counts[4 * c]) + " finite, " + std::to_string(counts[4 * c + 2]) +
		          " in the crop volume, " + std::to_string(counts[4 * c + 3]) + " points\n";
	report += "tolerance accuracy completeness f1\n";
	for (size_t k = 0; k < o.tolerances.size(); ++k) {
		const long long judged = free_space ? within_recon[k] + free_space[k] : used[0];   // observed space: the accurate and the free-space points
		const double a = judged ? (double)within_recon[k] / (double)judged : 0.0, c = used[1] ? (double)within_truth[k] / (double)used[1] : 0.0;
		const double f = a + c == 0.0 ? 0.0 : 2.0 * a * c / (a + c);
		snprintf(text, sizeof text, "%.9g %.6f %.6f %.6f\n", (double)o.tolerances[k], 100.0 * a, 100.0 * c, 100.0 * f);
		report += text;
	}
	if (free_space) {
		report += "tolerance accurate free_space unobserved\n";
		for (size_t k = 0; k < o.tolerances.size(); ++k) {
			snprintf(text, sizeof text, "%.9g %lld %lld %lld\n", (double)o.tolerances[k], within_recon[k], free_space[k], used[0] - within_recon[k] - free_space[k]);
			report += text;
		}
	}
	return report;
}

bool WritePlyVertices(const std::string& file, const std::vector<float>& xyz, std::string* error) {
	std::ofstream out(file, std::ios::binary);
	out << "ply\nformat binary_little_endian 1.0\nelement vertex " << xyz.size() / 3 << "\nproperty float x\nproperty float y\nproperty float z\nend_header\n";
	out.write((const char*)xyz.data(), (std::streamsize)(xyz.size() * 4));   // (the hosts this runs on are little-endian, as ExportPointCloud assumes)
	if (!out.good()) { *error = "cannot write " + file; return false; }
	return true;
}

bool ParseRefineStages(const std::string& list, std::vector<dvpci::Stage>* stages, std::string* error) {
	stages->clear();
	std::stringstream in(list);
	std::string item;
	while (std::getline(in, item, ',')) {
		std::stringstream parts(item);
		std::string word[3], rest;
		double v[3];
		bool ok = std::getline(parts, word[0], ':') && std::getline(parts, word[1], ':') && std::getline(parts, word[2], ':') && !std::getline(parts, rest, ':');
		for (int k = 0; k < 3 && ok; ++k) {
			char* end = nullptr;
			v[k] = strtod(word[k].c_str(), &end);
			ok = !word[k].empty() && !*end;
		}
		if (ok) ok = v[2] >= -1e9 && v[2] <= 1e9 && v[2] == floor(v[2]);   // (a NaN fails; the cast below is then in range)
		if (!ok) { *error = "--refine-alignment takes VOXEL:DISTANCE:ITERATIONS separated by commas, got `" + item + "`"; return false; }
		stages->push_back(dvpci::Stage{ v[0], v[1], (int)v[2] });
	}
	if (stages->empty() || list.back() == ',') { *error = "--refine-alignment takes VOXEL:DISTANCE:ITERATIONS separated by commas, got `" + list + "`"; return false; }
	if (stages->size() > (size_t)dvpci::kMaxStages) { *error = "--refine-alignment takes at most 8 stages, got " + std::to_string(stages->size()); return false; }
	return true;
}

bool WriteTransformFile(const std::string& file, const double m[16], std::string* error) {
	std::ofstream out(file, std::ios::binary);
	char text[128];
	for (int r = 0; r < 4; ++r) {
		snprintf(text, sizeof text, "%.17g %.17g %.17g %.17g\n", m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
		out << text;
	}
	if (!out.good()) { *error = "cannot write " + file; return false; }
	return true;
}

std::string AlignmentReport(const std::vector<dvpci::LogRecord>& log, const double m[16]) {
	std::string report;
	char text[256];
	for (size_t k = 0; k < log.size(); ++k) {
		if (k + 1 < log.size() && log[k + 1].stage == log[k].stage) continue;   // the stage's last step speaks for it
		snprintf(text, sizeof text, "alignment stage %d: %d steps, %lld of %lld correspondences, rmse %.9g\n", log[k].stage, log[k].step, log[k].n, log[k].n_src, log[k].rmse);
		report += text;
	}
	for (int r = 0; r < 4; ++r) {
		snprintf(text, sizeof text, "alignment %.17g %.17g %.17g %.17g\n", m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
		report += text;
	}
	return report;
}

static bool EvaluateCloudsOrThrow(const EvaluateOptions& o, std::string* report, std::string* error);

bool EvaluateClouds(const EvaluateOptions& o, std::string* report, std::string* error) {
	try {
		return EvaluateCloudsOrThrow(o, report, error);
	} catch (const std::bad_alloc&) {   // the clouds, or the host flavour's table, do not fit the host's memory
		*error = "out of host memory";
		return false;
	}
}

// the C ABI's view of a description (it points into `p`)
static dvp_cloud_prep AbiPrep(const dvpcp::Prep& p) {
	dvp_cloud_prep c;
	c.transform = p.has_transform ? p.m : nullptr;
	c.crop_axis = p.crop_axis;
	c.axis_min = p.axis_min;
	c.axis_max = p.axis_max;
	c.polygon_xyz = p.polygon.empty() ? nullptr : p.polygon.data();
	c.num_polygon = (int)(p.polygon.size() / 3);
	c.voxel = p.voxel;
	return c;
}

static bool EvaluateCloudsOrThrow(const EvaluateOptions& given, std::string* report, std::string* error) {
	EvaluateOptions o = given;
	const bool against_scans = !o.truth_scans.empty();
	if (against_scans) o.truth = o.truth_scans;   // (the report's ground_truth line names the project)
	const bool prepares = o.prepares();
	if (!o.save_prepared.empty() && !prepares) { *error = "--save-prepared needs --transform, --crop or --voxel-size"; return false; }
	if (!o.save_transform.empty() && o.refine.empty()) { *error = "--save-transform needs --refine-alignment"; return false; }
	dvpcp::Prep prep[2];   // recon, truth
	if (!o.transform_file.empty()) {
		if (!ReadTransformFile(o.transform_file, prep[0].m, error)) return false;
		prep[0].has_transform = true;
	}
	if (!o.crop_file.empty()) {
		if (!ReadCropFile(o.crop_file, &prep[0], error)) return false;
		prep[1].crop_axis = prep[0].crop_axis;
		prep[1].axis_min = prep[0].axis_min;
		prep[1].axis_max = prep[0].axis_max;
		prep[1].polygon = prep[0].polygon;
	}
	prep[0].voxel = prep[1].voxel = o.voxel;
	for (int c = 0; c < 2 && prepares; ++c) {
		const std::string what = dvpcp::check_prep(prep[c]);
		if (!what.empty()) { *error = what; return false; }
	}
	std::vector<float> recon, truth;
	std::vector<std::vector<float>> scan_points;
	std::vector<dvpcs::Scan> scans;
	std::string scan_lines;
	long long scan_total = 0;
	if (!ReadPlyVertices(o.recon, &recon, error)) return false;
	if (against_scans) {
		const std::string cube = dvpcs::check_cube(o.cube_size);
		if (!cube.empty()) { *error = cube; return false; }
		std::vector<ScanEntry> entries;
		if (!ReadScanProject(o.truth_scans, &entries, error)) return false;
		scan_points.resize(entries.size());
		scans.resize(entries.size());
		for (size_t s = 0; s < entries.size(); ++s) {
			std::string why;
			if (!ReadPlyVertices(entries[s].path, &scan_points[s], &why)) { *error = "scan " + entries[s].name + ": " + why; return false; }
			scans[s].xyz = scan_points[s].data();
			scans[s].num = (long long)(scan_points[s].size() / 3);
			for (int k = 0; k < 16; ++k) scans[s].m[k] = entries[s].m[k];
			float at[3];
			scans[s].scanner(at);
			char text[160];
			snprintf(text, sizeof text, ": %lld points, scanner at %.9g %.9g %.9g\n", scans[s].num, (double)at[0], (double)at[1], (double)at[2]);
			scan_lines += "scan " + entries[s].name + text;
		}
		const std::string what = dvpcs::check_scans(scans.data(), (int)scans.size(), &scan_total);
		if (!what.empty()) { *error = what; return false; }
		// the truth cloud on the host where something other than the evaluation itself reads it: the stages, the saved cloud
		if (!o.refine.empty() || (o.on_gpu && !o.save_prepared.empty())) dvpcs::serial_truth(scans.data(), (int)scans.size(), &truth);
	} else if (!ReadPlyVertices(o.truth, &truth, error)) return false;
	const std::vector<float>* cloud[2] = { &recon, &truth };
	const long long num[2] = { (long long)(recon.size() / 3), against_scans ? scan_total : (long long)(truth.size() / 3) };
	const int K = (int)o.tolerances.size();
	std::string alignment;
	if (!o.refine.empty()) {   // the stages first: prep[0]'s matrix becomes the refined one
		std::vector<dvpci::LogRecord> log;
		double M[16];
		for (int k = 0; k < 16; ++k) M[k] = prep[0].m[k];
		if (o.on_gpu) {
			const dvp_cloud_prep abi[2] = { AbiPrep(prep[0]), AbiPrep(prep[1]) };
			std::vector<dvp_icp_stage> stages;
			int capacity = 0, count = 0;
			for (const dvpci::Stage& s : o.refine) {
				stages.push_back(dvp_icp_stage{ s.voxel, s.max_distance, s.max_iterations });
				capacity += s.max_iterations > 0 && s.max_iterations <= dvpci::kMaxIterations ? s.max_iterations : 0;
			}
			std::vector<dvp_icp_log> records((size_t)capacity + 1);
			if (dvp_cloud_refine_alignment(o.device, recon.data(), num[0], truth.data(), num[1], &abi[0], &abi[1], stages.data(), (int)stages.size(), M, records.data(), capacity,
			                               &count) != 0) {
				*error = dvp_cloud_icp_last_error();
				return false;
			}
			for (int k = 0; k < count && k < capacity; ++k) log.push_back(dvpci::LogRecord{ records[(size_t)k].stage, records[(size_t)k].step, records[(size_t)k].n_src, records[(size_t)k].n, records[(size_t)k].rmse });
		} else {
			dvpci::HostBackend be;
			be.xyz[0] = recon.data(); be.xyz[1] = truth.data();
			be.num[0] = num[0]; be.num[1] = num[1];
			for (int c = 0; c < 2; ++c) {
				be.prep[c] = prep[c];
				be.prep[c].voxel = 0.0;
			}
			be.R = dvpci::cells_radius_from_environment();
			std::string what = be.R ? "" : "DVP_CLOUD_ICP_CELLS takes 27 or 125";
			if (what.empty()) what = dvpci::refine(be, o.refine.data(), (int)o.refine.size(), M, &log);
			if (!what.empty()) { *error = what; return false; }
		}
		for (int k = 0; k < 16; ++k) prep[0].m[k] = M[k];
		prep[0].has_transform = true;
		const std::string what = dvpcp::check_prep(prep[0]);
		if (!what.empty()) { *error = "the refined alignment: " + what; return false; }
		if (!o.save_transform.empty() && !WriteTransformFile(o.save_transform, M, error)) return false;
		alignment = AlignmentReport(log, M);
	}
	long long within_recon[dvpce::kMaxTolerances] = {}, within_truth[dvpce::kMaxTolerances] = {}, used[2] = { 0, 0 }, counts[8] = {}, free_space[dvpce::kMaxTolerances] = {};
	std::vector<float> prepared[2];
	if (against_scans && o.on_gpu) {
		const dvp_cloud_prep abi[2] = { AbiPrep(prep[0]), AbiPrep(prep[1]) };
		std::vector<dvp_cloud_scan> list(scans.size());
		for (size_t s = 0; s < scans.size(); ++s) {
			list[s].xyz = scans[s].xyz;
			list[s].num = scans[s].num;
			for (int k = 0; k < 16; ++k) list[s].transform[k] = scans[s].m[k];
		}
		if (dvp_cloud_evaluate_scans(o.device, recon.data(), num[0], prepares ? &abi[0] : nullptr, list.data(), (int)list.size(), prepares ? &abi[1] : nullptr, o.cube_size,
		                             o.tolerances.data(), K, within_recon, within_truth, used, free_space, counts, nullptr, nullptr) != 0) {
			*error = dvp_cloud_scan_last_error();
			return false;
		}
		for (int c = 0; c < 2 && !o.save_prepared.empty(); ++c) {
			prepared[c].resize(cloud[c]->size());
			long long again[4];
			if (dvp_cloud_prepare(o.device, cloud[c]->data(), num[c], &abi[c], prepared[c].data(), nullptr, again) != 0) { *error = dvp_cloud_prep_last_error(); return false; }
			prepared[c].resize((size_t)again[3] * 3);
		}
	} else if (against_scans) {
		const std::string what = K > dvpce::kMaxTolerances ? "at most 8 tolerances" : dvpcs::serial_evaluate_scans(recon.data(), num[0], prepares ? &prep[0] : nullptr, scans.data(), (int)scans.size(),
		                                   prepares ? &prep[1] : nullptr, o.cube_size, o.tolerances.data(), K, within_recon, within_truth, used, free_space, counts, prepared, nullptr, nullptr);
		if (!what.empty()) { *error = what; return false; }
	} else if (o.on_gpu && !prepares) {
		if (dvp_cloud_evaluate(o.device, recon.data(), num[0], truth.data(), num[1], o.tolerances.data(), K, within_recon, within_truth, used, nullptr, nullptr) != 0) {
			*error = dvp_cloud_last_error();
			return false;
		}
	} else if (o.on_gpu) {
		const dvp_cloud_prep abi[2] = { AbiPrep(prep[0]), AbiPrep(prep[1]) };
		if (dvp_cloud_evaluate_prepared(o.device, recon.data(), num[0], &abi[0], truth.data(), num[1], &abi[1], o.tolerances.data(), K, within_recon, within_truth, used, nullptr,
		                                nullptr, counts) != 0) {
			*error = dvp_cloud_prep_last_error();
			return false;
		}
		for (int c = 0; c < 2 && !o.save_prepared.empty(); ++c) {   // the prepared points themselves are only fetched to be saved
			prepared[c].resize(cloud[c]->size());
			long long again[4];
			if (dvp_cloud_prepare(o.device, cloud[c]->data(), num[c], &abi[c], prepared[c].data(), nullptr, again) != 0) { *error = dvp_cloud_prep_last_error(); return false; }
			prepared[c].resize((size_t)again[3] * 3);
		}
	} else {
		std::string what = K > dvpce::kMaxTolerances ? "at most 8 tolerances" : "";
		for (int c = 0; c < 2 && prepares && what.empty(); ++c) what = dvpcp::serial_prepare(cloud[c]->data(), num[c], prep[c], &prepared[c], nullptr, counts + 4 * c);
		if (what.empty()) {
			const std::vector<float>& r = prepares ? prepared[0] : recon, &t = prepares ? prepared[1] : truth;
			what = dvpce::serial_evaluate(r.data(), (long long)(r.size() / 3), t.data(), (long long)(t.size() / 3), o.tolerances.data(), K, within_recon, within_truth, used, nullptr, nullptr);
		}
		if (!what.empty()) { *error = what; return false; }
	}
	if (!o.save_prepared.empty() && (!WritePlyVertices(o.save_prepared + "recon.ply", prepared[0], error) || !WritePlyVertices(o.save_prepared + "truth.ply", prepared[1], error))) return false;
	*report = alignment + EvaluateReport(o, num, used, within_recon, within_truth, prepares ? counts : nullptr, scan_lines, against_scans ? free_space : nullptr);
	if (!o.out.empty()) {
		std::ofstream out(o.out, std::ios::binary);
		out << *report;
		if (!out.good()) { *error = "cannot write " + o.out; return false; }
	}
	return true;
}
