"""TEST INFRASTRUCTURE — ctypes wrapper of tests/sweep_list_host/sweep_list_emul.cpp: the host emulation (same interface as
tests.emul.emul.Emul) with the sweep site as view-compacted passes whose evaluation launches take the form the engine chooses —
per-view (pixel, view) lists or the pixels of the tile form — and the test hook of dvp_forms.hpp's sweep_eval_form."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import oracle as _o

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-s", "-C", _HERE, "libdvp_sweep_list_emul.so"])
        L = _o.bind_cpu_engine(ctypes.CDLL(os.path.join(_HERE, "libdvp_sweep_list_emul.so")), "emu_")
        L.swl_read_switches.argtypes = [ctypes.c_void_p]
        L.swl_run_passes.argtypes = [ctypes.c_void_p]
        L.swl_sweep_field.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.swl_stage1_lists.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.swl_stage1_lists.restype = ctypes.c_longlong
        _LIB = L
    return _LIB


class SweepListEmul(_o.Oracle):
    def __init__(self, width, height, num_images):
        super().__init__(width, height, num_images, _lib=lib(), _prefix="emu_")

    def read_switches(self):
        """DVP_SWEEP_ALL_SLOTS as the environment has it now (the engine reads it when a context is created)"""
        lib().swl_read_switches(self.h)

    def run_passes(self):
        """DepthToWeak + LocalRefine as view-compacted passes; returns the evaluation launches' form (0 tiles, 1 lists)"""
        form = lib().swl_run_passes(self.h)
        assert form >= 0
        return form

    def sweep_field(self, v, f):
        out = np.empty(self.W * self.H, np.float32)
        assert lib().swl_sweep_field(self.h, v, f, out.ctypes.data_as(ctypes.c_void_p)) == 0
        return out


def stage1_lists(S, L):
    """(flags [L], [list of view 0, ...]) of the last run_passes that built stage-1 lists: the flags its decide1 left, and the lists"""
    n = (ctypes.c_int * S)()
    fn = lib().swl_stage1_lists
    total = fn(S, n, None, None)
    assert total >= 0
    flags, lists = np.empty(L, np.int32), np.empty(max(total, 1), np.uint32)
    fn(S, n, flags.ctypes.data_as(ctypes.c_void_p), lists.ctypes.data_as(ctypes.c_void_p))
    at = np.concatenate([[0], np.cumsum(list(n))])
    return flags, [lists[at[v]:at[v + 1]] for v in range(S)]


def sweep_eval_form(fused, geom, wpr, sweep_fits, W, H, list_fits):
    """(DVP_SWEEP_LIST as read, dvp_forms.hpp: sweep_eval_form) under the environment as it stands"""
    a = (ctypes.c_int * 7)(fused, geom, wpr, sweep_fits, W, H, list_fits)
    out = (ctypes.c_int * 2)()
    lib().swl_forms_sweep_eval(a, out)
    return out[0], out[1]
