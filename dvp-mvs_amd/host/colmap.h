// colmap.h — `apd --convert-from`: a COLMAP model turned into the folder `apd` reads (images/%08d.jpg, cams/%08d_cam.txt, pair.txt,
// sfm/%08d.txt), what the reference's colmap2mvsnet.py does with OpenCV and numpy.  host/colmap.cpp; DESIGN.md section 7.
#ifndef DVP_HOST_COLMAP_H_
#define DVP_HOST_COLMAP_H_
#include "main.h"

struct ColmapCamera {
	int id = 0;
	std::string model;
	long long width = 0, height = 0;
	std::vector<double> params;
};
struct ColmapImage {
	int id = 0, camera_id = 0;
	double q[4] = { 0, 0, 0, 0 }, t[3] = { 0, 0, 0 };
	std::string name;
	std::vector<double> xy;              // 2 per observation
	std::vector<long long> point_ids;    // -1: no point
	std::string where;                   // "images.txt:12" / "images.bin: record 3", for messages
};
struct ColmapPoint {
	long long id = 0;
	double xyz[3] = { 0, 0, 0 };
	int rgb[3] = { 0, 0, 0 };
};
struct ColmapModel {
	std::vector<ColmapCamera> cameras;
	std::vector<ColmapImage> images;     // in order of COLMAP image id: index = the new number
	std::vector<ColmapPoint> points;
};
// cameras, images and points3D of `dir` in the format `ext` (".txt" or ".bin").  false: *error names the file and the line or record.
bool ReadColmapModel(const path& dir, const std::string& ext, ColmapModel* model, std::string* error);

struct ConvertOptions {
	path colmap_folder, save_folder;
	std::string model_dir = "dslr_calibration_undistorted", model_ext = ".txt";
	double scale_factor = 1, interval_scale = 1;
	int max_d = 192;
	bool sfm = true;        // write sfm/<id>.txt
	bool on_gpu = true;     // the scores, the JPEG reconstruction and the resampling on `device`; false: the same text on the host
	bool images = true;     // false: pair.txt, cams/ and sfm/ only (needs no device)
	bool undistort = false; // true: every picture resampled into the pinhole camera of its COLMAP camera, sfm/ written for that picture (csrc/dvp_undistort.hpp)
	int device = 0;
};
// Replaces files of the same names under save_folder and deletes nothing.  false: *error says what stopped it.
bool ConvertColmap(const ConvertOptions& options, std::string* error);

// What the converter computes before it writes, for callers that compare rather than read files back
struct ConvertedCameras {
	std::vector<double> extrinsic;   // 16 per image, row-major
	std::vector<double> intrinsic;   // 9 per image
	std::vector<double> depth;       // depth_min, interval, depth_num, depth_max per image
	std::vector<double> centres;     // 3 per image
};
bool ConvertCameras(const ColmapModel& model, const ConvertOptions& options, ConvertedCameras* out, std::string* error);
// Python's str(float) of a binary64: shortest digits that read back, ".0" or an exponent always, exponent form below 1e-4 and from 1e16
std::string PyFloatStr(double v);
// the rows of pair.txt for an n x n score matrix: min(20, n - 1) entries per view, by descending score, ties by descending index
std::string PairText(const uint32_t* score, int n);
#endif
