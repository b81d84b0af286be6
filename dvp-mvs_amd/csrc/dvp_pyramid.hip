// dvp_pyramid.hip — the level images on the device: what load_image (host/APD.cpp) makes on the host for every pyramid level —
// uint8 -> float, zero padding / cropping to the reference's size, cv::resize(INTER_LINEAR) — as one launch over all images of a
// context, from decoded bytes that were uploaded once per job (the dvp_images store).  The arithmetic lives in dvp_pyramid.hpp.
// A lane reads at most four bytes and stores one float; no LDS.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_pyramid.hpp"
#include "dvp_pyramid_run.h"

namespace dvppyr {

// a wave is 64 x-adjacent level pixels, blockIdx.z the image: rows of the planes are written coalesced
__global__ void __launch_bounds__(256) dvp_pyr_levels(const Sources images, int pad_w, int pad_h, double sx, double sy, float* __restrict__ out, int lw, int lh, int pitch,
                                                      size_t plane_stride) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= lw || y >= lh) return;
	const Source& im = images.v[blockIdx.z];
	out[(size_t)blockIdx.z * plane_stride + (size_t)y * pitch + x] = level_texel(im.bytes, (size_t)im.pitch, im.sw, im.sh, pad_w, pad_h, sx, sy, x, y);
}

int launch_levels(hipStream_t stream, const Sources& images, int n, int pad_w, int pad_h, int lw, int lh, float* interior, int pitch, size_t plane_stride) {
	hipLaunchKernelGGL(dvp_pyr_levels, dim3((unsigned)((lw + 63) / 64), (unsigned)((lh + 3) / 4), (unsigned)n), dim3(64, 4), 0, stream, images, pad_w, pad_h,
	                   (double)pad_w / lw, (double)pad_h / lh, interior, lw, lh, pitch, plane_stride);
	return hipGetLastError() != hipSuccess;
}

}   // namespace dvppyr

struct dvp_images {
	struct Entry { dvpmem::DevBlock bytes; int w = 0, h = 0; };   // w bytes per row; the map owns its images
	int device = 0;
	hipStream_t stream = nullptr;   // the copies of put and the work of level
	mutable std::shared_mutex m;    // entries, bytes
	std::map<int, Entry> entries;
	long long bytes = 0;
};

static thread_local dvpmem::CallError t_images_error;
static int images_fail(const char* who, const std::string& what) { return t_images_error.fail(who, what); }
static bool size_ok(int n) { return n >= 1 && n <= 32767; }

namespace dvppyr {

int store_device(const dvp_images* store) { return store->device; }

int store_sources(const dvp_images* store, const int* ids, int n, Sources* out, std::string* error) {
	std::shared_lock<std::shared_mutex> lock(store->m);
	for (int i = 0; i < n; ++i) {
		const auto it = store->entries.find(ids[i]);
		if (it == store->entries.end()) { *error = "image id " + std::to_string(ids[i]) + " is not in the store"; return 1; }
		out->v[i] = Source{ it->second.bytes.as<uint8_t>(), it->second.w, it->second.h, (long long)it->second.w };
	}
	return 0;
}

bool store_has(const dvp_images* store, int id) {
	std::shared_lock<std::shared_mutex> lock(store->m);
	return store->entries.count(id) != 0;
}

int store_adopt(dvp_images* store, int id, dvpmem::DevBlock& bytes, int w, int h) {
	std::unique_lock<std::shared_mutex> lock(store->m);
	if (store->entries.count(id)) return 1;
	dvp_images::Entry& e = store->entries[id];
	e.bytes = std::move(bytes);
	e.w = w;
	e.h = h;
	store->bytes += (long long)w * h;
	return 0;
}

}   // namespace dvppyr

extern "C" const char* dvp_images_last_error(void) { return t_images_error.c_str(); }

extern "C" int dvp_images_create(int device, dvp_images** out) {
	t_images_error.clear();
	if (!out) return images_fail("dvp_images_create", "the output pointer is required");
	*out = nullptr;
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return images_fail("dvp_images_create", "hipSetDevice failed"); }
	dvp_images* store = new dvp_images();
	store->device = device;
	if (hipStreamCreateWithFlags(&store->stream, hipStreamNonBlocking) != hipSuccess) {
		(void)hipGetLastError();
		delete store;
		return images_fail("dvp_images_create", "hipStreamCreate failed");
	}
	*out = store;
	return 0;
}

extern "C" int dvp_images_destroy(dvp_images* store) {
	t_images_error.clear();
	if (!store) return 0;
	(void)hipSetDevice(store->device);
	(void)hipStreamSynchronize(store->stream);
	(void)hipStreamDestroy(store->stream);
	delete store;   // frees the images
	return 0;
}

extern "C" int dvp_images_put(dvp_images* store, int id, const uint8_t* grey, int width, int height, long long pitch_bytes) {
	const char* who = "dvp_images_put";
	t_images_error.clear();
	if (!store || !grey) return images_fail(who, "the store and the image are required");
	if (!size_ok(width) || !size_ok(height) || pitch_bytes < width) return images_fail(who, "bad image geometry (sizes of 1 ... 32767, pitch >= width)");
	{
		std::shared_lock<std::shared_mutex> lock(store->m);
		if (store->entries.count(id)) return images_fail(who, "image id " + std::to_string(id) + " is already in the store");
	}
	// the copy runs without the lock: uploads and puts of other ids go on meanwhile
	if (hipSetDevice(store->device) != hipSuccess) { (void)hipGetLastError(); return images_fail(who, "hipSetDevice failed"); }
	dvp_images::Entry e;
	e.w = width;
	e.h = height;
	if (e.bytes.reserve((size_t)width * height)) return images_fail(who, "out of device memory");
	if (hipMemcpy2DAsync(e.bytes.as<uint8_t>(), (size_t)width, grey, (size_t)pitch_bytes, (size_t)width, (size_t)height, hipMemcpyHostToDevice, store->stream) != hipSuccess ||
	    hipStreamSynchronize(store->stream) != hipSuccess) {
		(void)hipGetLastError();
		return images_fail(who, "upload failed");
	}
	std::unique_lock<std::shared_mutex> lock(store->m);
	if (!store->entries.try_emplace(id, std::move(e)).second) {   // two threads put the same id: e keeps its block,
		lock.unlock();                                            // which is freed at the return, without the lock
		return images_fail(who, "image id " + std::to_string(id) + " is already in the store");
	}
	store->bytes += (long long)width * height;
	return 0;
}

extern "C" int dvp_images_drop(dvp_images* store, int id) {
	const char* who = "dvp_images_drop";
	t_images_error.clear();
	if (!store) return images_fail(who, "the store is required");
	dvp_images::Entry e;
	{
		std::unique_lock<std::shared_mutex> lock(store->m);
		const auto it = store->entries.find(id);
		if (it == store->entries.end()) return images_fail(who, "image id " + std::to_string(id) + " is not in the store");
		e = std::move(it->second);
		store->entries.erase(it);
		store->bytes -= (long long)e.w * e.h;
	}
	(void)hipSetDevice(store->device);
	return 0;   // e is freed here, without the lock
}

extern "C" int dvp_images_size(const dvp_images* store, int id, int* width, int* height) {
	const char* who = "dvp_images_size";
	t_images_error.clear();
	if (!store) return images_fail(who, "the store is required");
	std::shared_lock<std::shared_mutex> lock(store->m);
	const auto it = store->entries.find(id);
	if (it == store->entries.end()) return images_fail(who, "image id " + std::to_string(id) + " is not in the store");
	if (width) *width = it->second.w;
	if (height) *height = it->second.h;
	return 0;
}

extern "C" long long dvp_images_bytes(const dvp_images* store) {
	if (!store) return 0;
	std::shared_lock<std::shared_mutex> lock(store->m);
	return store->bytes;
}

extern "C" int dvp_images_level(dvp_images* store, int id, int pad_w, int pad_h, int level_w, int level_h, float* host_out) {
	const char* who = "dvp_images_level";
	t_images_error.clear();
	if (!store || !host_out) return images_fail(who, "the store and the output pointer are required");
	if (!size_ok(level_w) || !size_ok(level_h)) return images_fail(who, "bad level size (1 ... 32767)");
	if ((pad_w == 0) != (pad_h == 0) || (pad_w != 0 && (!size_ok(pad_w) || !size_ok(pad_h)))) return images_fail(who, "bad canvas size (1 ... 32767, or 0 x 0 for the image's own)");
	dvppyr::Sources src;
	std::string message;
	if (dvppyr::store_sources(store, &id, 1, &src, &message)) return images_fail(who, message);
	if (pad_w == 0) { pad_w = src.v[0].sw; pad_h = src.v[0].sh; }
	if (hipSetDevice(store->device) != hipSuccess) { (void)hipGetLastError(); return images_fail(who, "hipSetDevice failed"); }
	const size_t L = (size_t)level_w * level_h;
	dvpmem::DevBlock level;
	if (level.reserve(L * sizeof(float))) return images_fail(who, "out of device memory");
	int rc = dvppyr::launch_levels(store->stream, src, 1, pad_w, pad_h, level_w, level_h, level.as<float>(), level_w, L);
	if (!rc) rc = hipMemcpyAsync(host_out, level.as<float>(), L * sizeof(float), hipMemcpyDeviceToHost, store->stream) != hipSuccess || hipStreamSynchronize(store->stream) != hipSuccess;
	if (rc) (void)hipGetLastError();
	return rc ? images_fail(who, "the level could not be made or fetched") : 0;
}
