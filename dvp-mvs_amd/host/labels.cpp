// labels.cpp — the label half of the priors: EdgeSegment(scale, image, mode = 1) of the reference
// (/root/reference/APD.cpp:120-136, 348-401, 437-499) without OpenCV.
//
// What it computes.  Low-texture regions of the image become labelled segments; the anchor search and the
// RANSAC of the weak-pixel path use the label map to extend anchors along region boundaries and to prefer
// planes that agree with the anchors' normals (APD.cu:3455-3560, 3625).  Steps:
//   1. the grey image is halved twice (bilinear), a Roberts-cross gradient is thresholded at 4: white =
//      textured, black = flat;
//   2. black pixels are grouped into 4-connected regions (Connect + Label_Update); around every region of
//      at least `weak_tex_num` pixels the one-pixel outline is traced and straight segments in it are
//      found with the progressive probabilistic Hough transform, then drawn white into the texture map —
//      this closes gaps in the outline of flat regions so that two walls meeting at a faint corner do not
//      merge;
//   3. the map is resized to the working resolution, re-thresholded, its frame is cleaned like the edge
//      map's, black pixels are grouped again: label 0 = textured, k >= 1 = a flat region, -1 = a flat region
//      of at most `weak_tex_num` pixels.
// cv::resize, cv::HoughLinesP and cv::line are third-party arithmetic (OpenCV >= 3.3, absent here): restated
// from their documented algorithms (Matas et al.'s PPHT with OpenCV's multiply-with-carry generator;
// 8-connected Bresenham line).  PARITY UNPINNED — there is no OpenCV to compare with.
#include "APD.h"
#include <vector>

#include "../csrc/dvp_labels_mid.hpp"   // the outlines, the Hough transform and the lines: one text with the engine library

namespace {

Mat to_float(const Mat& u8) {
	Mat f(u8.rows, u8.cols, CV_32FC1);
	for (int r = 0; r < u8.rows; ++r) {
		const uint8_t* s = u8.ptr<uint8_t>(r);
		float* d = f.ptr<float>(r);
		for (int c = 0; c < u8.cols; ++c) d[c] = s[c];
	}
	return f;
}
Mat to_u8(const Mat& f) {   // round to nearest, saturate
	Mat u(f.rows, f.cols, CV_8UC1);
	for (int r = 0; r < f.rows; ++r) {
		const float* s = f.ptr<float>(r);
		uint8_t* d = u.ptr<uint8_t>(r);
		for (int c = 0; c < f.cols; ++c) d[c] = (uint8_t)std::min(255L, std::max(0L, std::lrintf(s[c])));
	}
	return u;
}
Mat resize_u8(const Mat& u8, int cols, int rows) {
	if (cols == u8.cols && rows == u8.rows) return u8.clone();
	return to_u8(ResizeLinear(to_float(u8), cols, rows));
}
void binarise(Mat& m, int thr) {   // cv::threshold(THRESH_BINARY)
	for (size_t i = 0, n = (size_t)m.rows * m.cols; i < n; ++i) m.data[i] = m.data[i] > thr ? 255 : 0;
}

// Roberts cross on the interior, 50/50 on the frame (APD.cpp:120-136)
Mat RobertsCross(const Mat& src) {
	Mat dst(src.rows, src.cols, CV_8UC1);
	for (int i = 0; i < src.rows; ++i)
		for (int j = 0; j < src.cols; ++j) {
			int t1 = 50, t2 = 50;
			if (i > 0 && i < src.rows - 1 && j > 0 && j < src.cols - 1) {
				t1 = src.at<uint8_t>(i, j) - src.at<uint8_t>(i + 1, j + 1);
				t2 = src.at<uint8_t>(i + 1, j) - src.at<uint8_t>(i, j + 1);
			}
			dst.at<uint8_t>(i, j) = (uint8_t)std::sqrt((double)(t1 * t1 + t2 * t2));
		}
	return dst;
}

}  // namespace

// EdgeSegment(scale, src_image, mode = 1, use_canny = false): CV_32SC1 label map at src size / 2^scale
Mat LabelSegment(const int scale, const Mat& src_image, LabelStages* stages) {
	const int robthr = 4;
	const int weak_tex_num = (int)(1.0 * src_image.rows * src_image.cols / (1024 << scale << scale));
	Mat quarter = resize_u8(src_image, src_image.cols / 2, src_image.rows / 2);
	quarter = resize_u8(quarter, quarter.cols / 2, quarter.rows / 2);
	const int unit = (int)(std::min(quarter.cols, quarter.rows) / 30.0);   // Hough threshold, minimum length and maximum gap
	Mat texture = RobertsCross(quarter);
	binarise(texture, robthr);
	if (stages) { stages->quarter = quarter.clone(); stages->texture = texture.clone(); stages->weak_tex_num = weak_tex_num; }
	{
		Mat region(texture.rows, texture.cols, CV_32S);
		std::vector<int> region_size;
		Connect(texture, region, region_size);
		Label_Update(region, region_size);
		// the large regions by number, everything else -1: the outlines, the transform and the lines are dvp_labels_mid.hpp's
		std::vector<int32_t> key((size_t)region.rows * region.cols);
		for (int y = 0; y < region.rows; ++y) {
			const int* row = region.ptr<int>(y);
			for (int x = 0; x < region.cols; ++x) key[(size_t)y * region.cols + x] = (row[x] != 0 && region_size[row[x]] >= weak_tex_num) ? row[x] : -1;
		}
		dvplabmid::DrawRegionLines(key.data(), region.cols, region.rows, unit, [&](int x, int y) { texture.at<uint8_t>(y, x) = 255; });
	}
	if (stages) stages->texture_lines = texture.clone();
	const float factor = 1.0f / (float)(1 << scale);
	Mat map = resize_u8(texture, (int)std::round(src_image.cols * factor), (int)std::round(src_image.rows * factor));
	binarise(map, robthr);
	if (stages) stages->resized = map.clone();
	const int rows = map.rows, cols = map.cols;
	uint8_t* D = map.data;   // frame clean-up (APD.cpp:452-463)
	for (int y = 0; y < rows; y++) {
		if (D[y * cols + 1] == 0) D[y * cols] = 0;
		if (D[y * cols + cols - 2] == 0) D[y * cols + cols - 1] = 0;
	}
	for (int x = 0; x < cols; x++) {
		if (D[1 * cols + x] == 0) D[0 * cols + x] = 0;
		if (D[(rows - 2) * cols + x] == 0) D[(rows - 1) * cols + x] = 0;
	}
	if (stages) stages->cleaned = map.clone();
	Mat label(rows, cols, CV_32S);
	std::vector<int> label_size;
	Connect(map, label, label_size);
	Label_Update(label, label_size);
	for (int y = 0; y < rows; ++y) {
		int* row = label.ptr<int>(y);
		for (int x = 0; x < cols; ++x)
			if (row[x] != 0 && label_size[row[x]] <= weak_tex_num) row[x] = -1;
	}
	return label;
}
