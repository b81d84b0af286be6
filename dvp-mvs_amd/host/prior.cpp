// prior.cpp — monocular-depth plane prior of a FIRST_INIT pass (/root/reference/APD.cpp:1210-1424).
//
// Inputs, per reference view:  dep/<id>.dmb   (BinMat f32, a relative depth map from Depth-Anything-V2;
//                                              the network itself is external and never part of this repo)
//                              sfm/<id>.txt   (one sparse SfM point per line: x2d y2d X Y Z r g b)
//                              cams/<id>_cam.txt
// What the reference does with them and this file restates:
//   1. dep <- 255 - dep                                                        (APD.cpp:1221-1225)
//   2. for every sparse point that projects inside the map: rate = dep(proj) / projected depth
//                                                                              (APD.cpp:1254-1268)
//   3. Delaunay-triangulate the 2-D positions; fill a rate map by barycentric interpolation inside
//      every triangle, `rates[n/2]` (the middle element, not a median) elsewhere (APD.cpp:1276-1350)
//   4. dep <- dep / rate map  (now metric), rescale to the working size        (APD.cpp:1352-1363)
//   5. normals from forward differences of the back-projected depth, flipped toward the camera and
//      rotated to the world frame; plane = (world normal, depth)               (APD.cpp:1365-1422)
// The debug pictures the reference writes on the way (COLMAP_*.jpg, Tri_*.jpg, depth_anything_*.jpg,
// normal_COLMAP.jpg) are not produced.
//
// The sequential part (points, Delaunay triangulation — a substitute for cv::Subdiv2D —, triangle list) is
// ../csrc/dvp_prior_mid.hpp and the per-pixel arithmetic ../csrc/dvp_prior.hpp: one text for this file and for the engine's
// device path (dvp_plane_prior, `apd --prior-on gpu`).
#include "APD.h"
#include "../csrc/dvp_prior_mid.hpp"

// APD.cpp:24-49
double calculateZ(const double A[3], const double B[3], const double C[3], double X, double Y) { return dvpprior::calculate_z(A, B, C, X, Y); }

// APD.cpp:51-80.  Points outside [0,cols)x[0,rows) are not inserted; triangle corners are the
// integer-truncated vertex positions; the three rates are looked up by exact coordinate match.
std::vector<Triangle> DelaunayTriangulation(int cols, int rows, const Rect boundRC, std::vector<float2> xy_temps, std::vector<float> rates) {
	std::vector<float> xy(2 * xy_temps.size());
	for (size_t i = 0; i < xy_temps.size(); ++i) { xy[2 * i] = xy_temps[i].x; xy[2 * i + 1] = xy_temps[i].y; }
	std::vector<Triangle> results;
	for (const dvpprior::Tri& t : dvppriormid::DelaunayCorners(cols, rows, boundRC.x, boundRC.y, boundRC.width, boundRC.height, xy.data(), rates.data(), xy_temps.size())) {
		Triangle tri(Point(t.x1, t.y1), Point(t.x2, t.y2), Point(t.x3, t.y3));
		tri.rate1 = t.r1; tri.rate2 = t.r2; tri.rate3 = t.r3;
		results.push_back(tri);
	}
	return results;
}

void ProjectCamera(const float3 PointX, const Camera camera, float2& point, float& depth) {   // APD.cpp:536-546
	const float X[3] = { PointX.x, PointX.y, PointX.z };
	dvppriormid::ProjectPoint(X, camera.K, camera.R, camera.t, &point.x, &point.y, &depth);
}

static std::vector<float> flat(const std::vector<float2>& v) {
	std::vector<float> out(2 * v.size());
	for (size_t i = 0; i < v.size(); ++i) { out[2 * i] = v[i].x; out[2 * i + 1] = v[i].y; }
	return out;
}
static std::vector<float> flat(const std::vector<float3>& v) {
	std::vector<float> out(3 * v.size());
	for (size_t i = 0; i < v.size(); ++i) { out[3 * i] = v[i].x; out[3 * i + 1] = v[i].y; out[3 * i + 2] = v[i].z; }
	return out;
}

// Steps 1-4: relative map + sparse points -> metric depth at the map's own resolution.
// `cam` is the camera as read from cams/<id>_cam.txt (unscaled, APD.cpp:1258-1260).
bool MetricDepthFromPrior(Mat& dep, const std::vector<float2>& xy, const std::vector<float3>& xyz, const Camera& cam) {
	if (dep.empty()) return false;
	float middle_rate = 0;
	std::vector<dvpprior::Tri> triangles;   // (from the map as read: the shared text forms 255 - dep at the points itself; a Mat's rows are dense)
	const bool usable = dvppriormid::PriorTriangles(dep.ptr<float>(0), dep.cols, dep.rows, flat(xy).data(), flat(xyz).data(), xy.size(), cam.K, cam.R, cam.t, &middle_rate, &triangles);
	for (int y = 0; y < dep.rows; y++)
		for (int x = 0; x < dep.cols; x++) dep.at<float>(y, x) = 255 - dep.at<float>(y, x);
	if (!usable) return false;
	Mat all_rate_map(dep.rows, dep.cols, CV_32FC1);
	for (int y = 0; y < dep.rows; y++)
		for (int x = 0; x < dep.cols; x++) all_rate_map.at<float>(y, x) = middle_rate;
	for (const auto& triangle : triangles) {
		const float step = triangle.step;
		// barycentric sweep of APD.cpp:1333-1347 (float loop counters, truncating pixel casts)
		for (float p = 0; p < 1.0; p += step) {
			for (float q = 0; q < 1.0 - p; q += step) {
				const int x = p * triangle.x1 + q * triangle.x2 + (1.0 - p - q) * triangle.x3;
				const int y = p * triangle.y1 + q * triangle.y2 + (1.0 - p - q) * triangle.y3;
				all_rate_map.at<float>(y, x) = dvpprior::rate_of(triangle, x, y);
			}
		}
	}
	for (int y = 0; y < dep.rows; y++)
		for (int x = 0; x < dep.cols; x++) dep.at<float>(y, x) /= all_rate_map.at<float>(y, x);
	return true;
}

// Step 5: planes (world normal, depth) from a metric depth map at the working size.
// Border pixels keep a zero normal (APD.cpp:1367-1368 loops over the interior only).
void PlanesFromDepth(const Mat& dep, const Camera& cam, float4* planes) {
	const int width = dep.cols, height = dep.rows;
	const float* map = dep.ptr<float>(0);   // (a Mat's rows are dense)
	for (int y = 0; y < height; ++y) {
		for (int x = 0; x < width; ++x) {
			const dvpprior::P4 pl = dvpprior::plane_at(map, width, height, cam.K, cam.R, x, y);
			planes[(size_t)y * width + x] = float4{ pl.x, pl.y, pl.z, pl.w };
		}
	}
}

// The inputs of one problem's prior as the files hold them: false when dep/, sfm/ or the camera is missing or unusable.
bool ReadPlanePriorInputs(const Problem& problem, Mat& dep, std::vector<float2>& xy, std::vector<float3>& xyz, Camera& cam) {
	const path dep_path = problem.dense_folder / path("dep") / path(ToFormatIndex(problem.ref_image_id) + ".dmb");
	const path sfm_path = problem.dense_folder / path("sfm") / path(ToFormatIndex(problem.ref_image_id) + ".txt");
	if (!std::filesystem::exists(dep_path) || !std::filesystem::exists(sfm_path)) return false;
	if (!ReadBinMat(dep_path, dep) || dep.empty() || dep.type() != CV_32FC1) return false;
	xy.clear();
	xyz.clear();
	{
		std::ifstream file(sfm_path);
		std::string line;
		while (std::getline(file, line)) {   // APD.cpp:1241-1250
			std::istringstream iss(line);
			float x_2d = 0, y_2d = 0, x_3d = 0, y_3d = 0, z_3d = 0;
			int r, g, b;
			iss >> x_2d >> y_2d >> x_3d >> y_3d >> z_3d >> r >> g >> b;
			xy.push_back(float2{ x_2d, y_2d });
			xyz.push_back(float3{ x_3d, y_3d, z_3d });
		}
	}
	return ReadCamera(problem.dense_folder / path("cams") / path(ToFormatIndex(problem.ref_image_id) + "_cam.txt"), cam);
}

// The whole block for one problem.  Returns false (planes untouched) when dep/ or sfm/ inputs are
// missing or unusable; the caller then leaves the planes at zero and RandomInitialization draws
// random ones (APD.cu:1289-1291) — the reference has no such fallback and reads an empty Mat.
bool BuildPlanePrior(const Problem& problem, const Camera& scaled_ref_camera, int width, int height, float4* planes) {
	Mat dep;
	std::vector<float2> xy;
	std::vector<float3> xyz;
	Camera cam;
	if (!ReadPlanePriorInputs(problem, dep, xy, xyz, cam)) return false;
	if (!MetricDepthFromPrior(dep, xy, xyz, cam)) return false;
	if (dep.cols != width || dep.rows != height) RescaleMatToTargetSize<float>(dep, dep, width, height);
	PlanesFromDepth(dep, scaled_ref_camera, planes);
	return true;
}
