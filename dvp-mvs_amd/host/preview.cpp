// preview.cpp — the preview files of `apd --previews` (the reference's show_medium_result, main.h:122): depth_<it>.jpg,
// normal_<it>.jpg, weak_<it>.jpg (ShowDepthMap / ShowNormalMap / ShowWeakImage, APD.cpp:694-812, rendered and encoded on the
// device: dvp_preview_begin), weak.png (main.cpp:383-384) and rawedge_<s>.jpg (main.cpp:219-223, dvp_jpeg_encode).
#include "APD.h"

#include <zlib.h>

// temporary name + rename, as the result store writes the maps: a reader of the folder never sees a torn file
bool WriteFileAtomic(const path& file, const void* data, size_t bytes) {
	path tmp = file;
	tmp += ".part";
	{
		std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
		if (!out) return false;
		out.write(static_cast<const char*>(data), (std::streamsize)bytes);
		if (!out) return false;
	}
	std::error_code ec;
	std::filesystem::rename(tmp, file, ec);
	return !ec;
}

// 8-bit RGB PNG (what cv::imwrite makes of the BGR weak image): filter 0 on every row, one zlib stream
bool WritePngRGB(const path& file, const uint8_t* rgb, int width, int height) {
	std::vector<uint8_t> raw((size_t)height * (1 + (size_t)width * 3));
	for (int r = 0; r < height; ++r) {
		uint8_t* row = raw.data() + (size_t)r * (1 + (size_t)width * 3);
		row[0] = 0;
		std::memcpy(row + 1, rgb + (size_t)r * width * 3, (size_t)width * 3);
	}
	uLongf zlen = compressBound((uLong)raw.size());
	std::vector<uint8_t> z(zlen);
	if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 1) != Z_OK) return false;
	std::vector<uint8_t> png = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
	auto chunk = [&png](const char* type, const uint8_t* d, size_t n) {
		for (int s = 24; s >= 0; s -= 8) png.push_back((uint8_t)(n >> s));
		const size_t at = png.size();
		png.insert(png.end(), type, type + 4);
		png.insert(png.end(), d, d + n);
		const uLong crc = crc32(0L, png.data() + at, (uInt)(n + 4));
		for (int s = 24; s >= 0; s -= 8) png.push_back((uint8_t)(crc >> s));
	};
	const uint8_t ihdr[13] = { (uint8_t)(width >> 24), (uint8_t)(width >> 16), (uint8_t)(width >> 8), (uint8_t)width,
	                           (uint8_t)(height >> 24), (uint8_t)(height >> 16), (uint8_t)(height >> 8), (uint8_t)height, 8, 2, 0, 0, 0 };
	chunk("IHDR", ihdr, 13);
	chunk("IDAT", z.data(), zlen);
	chunk("IEND", nullptr, 0);
	return WriteFileAtomic(file, png.data(), png.size());
}

// ShowWeakImage (APD.cpp:785-812) as weak.png: WEAK white, STRONG green, UNKNOWN red (RGB order in the file)
bool WriteWeakPng(const path& file, const Mat& weak) {
	std::vector<uint8_t> rgb((size_t)weak.rows * weak.cols * 3, 0);
	for (int r = 0; r < weak.rows; ++r) {
		const uint8_t* s = weak.ptr<uint8_t>(r);
		uint8_t* o = rgb.data() + (size_t)r * weak.cols * 3;
		for (int c = 0; c < weak.cols; ++c, o += 3) {
			if (s[c] == WEAK) { o[0] = 255; o[1] = 255; o[2] = 255; }
			else if (s[c] == STRONG) o[1] = 255;
			else if (s[c] == UNKNOWN) o[0] = 255;
		}
	}
	return WritePngRGB(file, rgb.data(), weak.cols, weak.rows);
}

// cv::imwrite of a CV_8UC1 map at quality 95, encoded on this driver's GPU
bool WriteGreyJpeg(const path& file, const Mat& grey) {
	if (grey.empty() || grey.type() != CV_8UC1) return false;
	const long long cap = dvp_jpeg_bound(grey.cols, grey.rows, 1);
	std::vector<uint8_t> out(cap > 0 ? (size_t)cap : 0);
	long long n = 0;
	if (dvp_jpeg_encode(APD::GetDevice(), grey.ptr<uint8_t>(0), grey.cols, grey.rows, 1, (long long)grey.step, 95, 0, out.data(), cap, &n) != 0) {
		std::cerr << "rawedge: " << dvp_jpeg_last_error() << std::endl;
		return false;
	}
	return WriteFileAtomic(file, out.data(), (size_t)n);
}
