"""TEST INFRASTRUCTURE — ctypes wrapper of tests/sweep_host/sweep_host.cpp: the host emulation (same interface as
tests.emul.emul.Emul) with the sweep site's DVP_SWEEP_ALL_SLOTS switch and a look at the passes' cost records."""
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
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = _o.bind_cpu_engine(ctypes.CDLL(os.path.join(_HERE, "libdvp_sweep_host.so")), "emu_")
        L.swh_read_switches.argtypes = [ctypes.c_void_p]
        L.swh_run_passes.argtypes = [ctypes.c_void_p]
        L.swh_sweep_field.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _LIB = L
    return _LIB


class SweepEmul(_o.Oracle):
    SITE = 100   # dvp_stages.hpp: kStageSweeps, the fused launch site of dvp_run_patchmatch

    def __init__(self, width, height, num_images):
        super().__init__(width, height, num_images, _lib=lib(), _prefix="emu_")

    def read_switches(self):
        """DVP_SWEEP_ALL_SLOTS as the environment has it now (the engine reads it when a context is created)"""
        lib().swh_read_switches(self.h)

    def run_site(self, passes):
        """DepthToWeak + LocalRefine as dvp_run_patchmatch's one launch site: the view-compacted passes, or the fused kernel"""
        if passes:
            assert lib().swh_run_passes(self.h) == 0
        else:
            assert self.L.ora_run_stage(self.h, self.SITE, 0, 0) == 0

    def sweep_field(self, v, f):
        out = np.empty(self.W * self.H, np.float32)
        assert lib().swh_sweep_field(self.h, v, f, out.ctypes.data_as(ctypes.c_void_p)) == 0
        return out
