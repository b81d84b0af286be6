"""REFERENCE PIN — TEST INFRASTRUCTURE ONLY (ctypes wrapper around oracle/_ref/libdvp_ref.so).

The library is the reference's own device text (APD.cu in front of APD::RunPatchMatch) compiled for the
host by oracle/make_ref.py, behind oracle/ref_harness.cpp.  `Reference` has the part of
oracle.Oracle's interface the tests use — same stage names, same buffer names and layouts — so one
launch can be run in both and every buffer compared.  Only tests/ may import this module.
"""
import ctypes
import os

import numpy as np

from . import make_ref
from .oracle import BUFFERS, STAGES, _p

_LIB = None


def library_path():
    return make_ref.LIB


def unavailable_reason():
    """None when the library can be loaded (built already, or buildable from the reference tree)."""
    if os.path.isfile(make_ref.LIB) or make_ref.available():
        return None
    return "oracle/_ref/libdvp_ref.so is absent and there is no reference tree at %s to build it from" % make_ref.reference_dir()


def lib():
    global _LIB
    if _LIB is None:
        if make_ref.available():
            make_ref.build()        # no-op when up to date
        L = ctypes.CDLL(make_ref.LIB)
        L.ref_create.restype = ctypes.c_void_p
        L.ref_create.argtypes = [ctypes.c_int] * 3
        L.ref_destroy.argtypes = [ctypes.c_void_p]
        for name in ("ref_set_image", "ref_set_depth"):
            getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.ref_set_cameras.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.ref_set_params.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.ref_set_seed.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.ref_set_sampler.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.ref_set_debug.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.ref_upload_state.argtypes = [ctypes.c_void_p] * 7
        L.ref_buffer_bytes.restype = ctypes.c_longlong
        L.ref_buffer_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.ref_get_buffer.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.ref_set_buffer.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.ref_weak_count.argtypes = [ctypes.c_void_p]
        L.ref_run_stage.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.ref_last_bad_line.argtypes = [ctypes.c_void_p]
        L.ref_violation.restype = ctypes.c_longlong
        L.ref_violation.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ref_homography.argtypes = [ctypes.c_void_p] * 4
        L.ref_corresponding_point.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        for name in ("ref_ncc_old", "ref_ncc_new", "ref_geom_cost"):
            f = getattr(L, name)
            f.restype = ctypes.c_float
            f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.ref_eval_cost_vectors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.ref_bresenham.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
        L.ref_point_in_triangle.argtypes = [ctypes.c_int] * 8
        _LIB = L
    return _LIB


class DrawError(RuntimeError):
    """a launch drew from a source line the draw table (oracle/ref_draws.json) does not key"""


class Reference:
    def __init__(self, width, height, num_images):
        self.L = lib()
        self.W, self.H, self.NI = width, height, num_images
        self.h = ctypes.c_void_p(self.L.ref_create(width, height, num_images))
        assert self.h

    def close(self):
        if self.h:
            self.L.ref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_images(self, images):
        for i in range(self.NI):
            a = np.ascontiguousarray(images[i], np.float32)
            assert a.shape == (self.H, self.W)
            self.L.ref_set_image(self.h, i, _p(a))

    def set_depths(self, depths):
        for i in range(self.NI):
            a = np.ascontiguousarray(depths[i], np.float32)
            assert a.shape == (self.H, self.W)
            self.L.ref_set_depth(self.h, i, _p(a))

    def set_cameras(self, cams):
        a = np.ascontiguousarray(cams)
        assert a.dtype.itemsize == 112
        self.L.ref_set_cameras(self.h, _p(a), len(a))

    def set_params(self, params):
        a = np.ascontiguousarray(params).reshape(1)
        assert a.dtype.itemsize == 76
        self.L.ref_set_params(self.h, _p(a))
        self.params = a

    def set_seed(self, seed):
        self.L.ref_set_seed(self.h, seed)

    def set_sampler(self, s):
        self.L.ref_set_sampler(self.h, s)

    def set_debug(self, on):
        """compare the whole state with the pre-launch snapshot after every thread (slow: tiny scenes only)"""
        self.L.ref_set_debug(self.h, int(on))

    def upload_state(self, planes=None, views=None, weak=None, edge=None, label=None, radius=None):
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        args = [c(planes, np.float32), c(views, np.uint32), c(weak, np.uint8), c(edge, np.uint8), c(label, np.int32), c(radius, np.int32)]
        self.L.ref_upload_state(self.h, *[_p(a) for a in args])

    def get(self, name):
        bid, dt, k = BUFFERS[name]
        nbytes = self.L.ref_buffer_bytes(self.h, bid)
        out = np.empty(nbytes // np.dtype(dt).itemsize, dt)
        r = self.L.ref_get_buffer(self.h, bid, _p(out))
        assert r == 0, "%s: the reference's candidate stride aliases for more than four source views" % name
        return out.reshape(-1, k) if k > 1 else out

    def set(self, name, arr):
        bid, dt, k = BUFFERS[name]
        a = np.ascontiguousarray(arr, dt)
        assert a.nbytes == self.L.ref_buffer_bytes(self.h, bid), (name, a.nbytes)
        r = self.L.ref_set_buffer(self.h, bid, _p(a))
        assert r == 0, name

    def weak_count(self):
        return self.L.ref_weak_count(self.h)

    def run_stage(self, name, it=0, colour=0):
        r = self.L.ref_run_stage(self.h, STAGES[name], it, colour)
        if r == -2:
            raise DrawError("%s(it=%d, colour=%d): draw from APD.cu:%d, which the draw table does not key"
                            % (name, it, colour, self.L.ref_last_bad_line(self.h)))
        assert r == 0

    def violation(self):
        """(threads that wrote outside their pixel's rows in the last launch, first such pixel, its buffer name) — debug switch"""
        px, buf = ctypes.c_int(-1), ctypes.c_int(-1)
        n = self.L.ref_violation(self.h, ctypes.byref(px), ctypes.byref(buf))
        names = {v[0]: k for k, v in BUFFERS.items()}
        return int(n), px.value, names.get(buf.value)

    # ---- function-level entry points ----
    def homography(self, ref_cam, src_cam, plane):
        a, b = np.ascontiguousarray(ref_cam).reshape(1), np.ascontiguousarray(src_cam).reshape(1)
        pl = np.ascontiguousarray(plane, np.float32)
        out = np.empty(9, np.float32)
        self.L.ref_homography(_p(a), _p(b), _p(pl), _p(out))
        return out

    def corresponding_point(self, Hm, x, y):
        a = np.ascontiguousarray(Hm, np.float32)
        out = np.empty(2, np.float32)
        self.L.ref_corresponding_point(_p(a), x, y, _p(out))
        return out

    def ncc_old(self, x, y, src_idx, plane):
        return self.L.ref_ncc_old(self.h, x, y, src_idx, _p(np.ascontiguousarray(plane, np.float32)))

    def ncc_new(self, x, y, src_idx, plane):
        return self.L.ref_ncc_new(self.h, x, y, src_idx, _p(np.ascontiguousarray(plane, np.float32)))

    def geom_cost(self, x, y, src_idx, plane):
        return self.L.ref_geom_cost(self.h, x, y, src_idx, _p(np.ascontiguousarray(plane, np.float32)))

    def eval_cost_vectors(self, px, planes):
        px = np.ascontiguousarray(px, np.int32)
        planes = np.ascontiguousarray(planes, np.float32)
        out = np.empty((len(px), self.NI - 1), np.float32)
        self.L.ref_eval_cost_vectors(self.h, _p(px), _p(planes), len(px), _p(out))
        return out

    def bresenham(self, a, b):
        return bool(self.L.ref_bresenham(self.h, int(a[0]), int(a[1]), int(b[0]), int(b[1])))

    def point_in_triangle(self, a, b, c, p):
        return bool(self.L.ref_point_in_triangle(int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(c[0]), int(c[1]), int(p[0]), int(p[1])))


def from_scene(scene, params, seed=1234, sampler=0, depths=None):
    r = Reference(scene["width"], scene["height"], len(scene["cameras"]))
    r.set_images(scene["images"])
    r.set_cameras(scene["cameras"])
    r.set_params(params)
    r.set_seed(seed)
    r.set_sampler(sampler)
    if depths is not None:
        r.set_depths(depths)
    return r
