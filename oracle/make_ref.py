"""Recipe of the reference pin: builds oracle/_ref/libdvp_ref.so from the reference's own device text.

The reference tree (DVP_REFERENCE_DIR, default /root/reference) is read, never copied into the
repository: the part of its APD.cu in front of the definition of APD::RunPatchMatch (the device
functions and the 16 kernels) is written, line numbers kept, into oracle/_ref/ together with APD.h and
main.h, and compiled there against the stand-in headers of oracle/ref_shim/ and oracle/ref_harness.cpp,
with the oracle Makefile's flags.  oracle/_ref/ is ignored by git.

It refuses to build when the three files are not the ones the draw table (ref_draws.json) and the line
citations of oracle/ were written against, or when the cuRAND call sites of the cut text are not
exactly the ones the table keys.

    python oracle/make_ref.py            # build (no-op when up to date)
    python oracle/make_ref.py --force
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT, "libdvp_ref.so")
TABLE = os.path.join(HERE, "ref_draws.json")
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mavx2", "-mfma", "-w"]
# RngSub of ora_common.h; DISCARD: see ref_draws.json
SUBS = {"SUB_VIEW": 0, "SUB_DEPTH_RAND": 1, "SUB_NORMAL": 2, "SUB_DEPTH_PERT": 3, "SUB_LIMIT": 4,
        "SUB_SEARCH": 5, "SUB_RANSAC": 6, "DISCARD": -1}
DRAW_CALL = re.compile(r"\bcurand(?:_uniform)?\s*\(")


def reference_dir():
    return os.environ.get("DVP_REFERENCE_DIR", "/root/reference")


def available():
    d = reference_dir()
    return all(os.path.isfile(os.path.join(d, n)) for n in ("APD.cu", "APD.h", "main.h"))


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _check_subs():
    """SUBS must be ora_common.h's enum."""
    text = open(os.path.join(HERE, "ora_common.h"), encoding="utf-8").read()
    for name, val in SUBS.items():
        if name == "DISCARD":
            continue
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        if not m or int(m.group(1)) != val:
            raise RuntimeError("make_ref: %s is not %d in ora_common.h" % (name, val))


def cut_device_text(lines):
    """Index of the line that defines APD::RunPatchMatch: everything in front of it is device text."""
    hits = [i for i, l in enumerate(lines) if re.match(r"\s*void\s+APD::RunPatchMatch\s*\(", l)]
    if len(hits) != 1:
        raise RuntimeError("make_ref: expected one definition of APD::RunPatchMatch, found %d" % len(hits))
    return hits[0]


def draw_sites(lines):
    """[(line number, call sites on it)] of the cut text, // comments left out."""
    sites = []
    for i, l in enumerate(lines):
        n = len(DRAW_CALL.findall(l.split("//", 1)[0]))
        if n:
            sites.append((i + 1, n))
    return sites


def check_table(table, lines):
    sites = draw_sites(lines)
    want = sum(d["calls"] for d in table["draws"])
    have = sum(n for _, n in sites)
    if want != have:
        raise RuntimeError("make_ref: the cut text has %d cuRAND call sites, the draw table keys %d" % (have, want))
    for d in table["draws"]:
        n = sum(c for ln, c in sites if d["first"] <= ln <= d["last"])
        if n != d["calls"]:
            raise RuntimeError("make_ref: lines %d-%d hold %d cuRAND call sites, the table says %d"
                               % (d["first"], d["last"], n, d["calls"]))
        if d["sub"] not in SUBS:
            raise RuntimeError("make_ref: unknown sub-stream %r" % d["sub"])


def build(force=False, verbose=False):
    """Builds the library; returns its path.  Raises when the reference is absent or not the pinned one."""
    if not available():
        raise RuntimeError("make_ref: no reference tree at %s" % reference_dir())
    _check_subs()
    ref = reference_dir()
    table = json.load(open(TABLE))
    shas = {}
    for name, key in (("APD.cu", "apd_cu_sha256"), ("APD.h", "apd_h_sha256"), ("main.h", "main_h_sha256")):
        shas[name] = _sha(os.path.join(ref, name))
        if shas[name] != table[key]:
            raise RuntimeError("make_ref: %s is not the pinned file (sha256 %s, expected %s)"
                               % (name, shas[name], table[key]))
    own = [os.path.join(HERE, "ref_harness.cpp"), TABLE, os.path.join(HERE, "ora_common.h"), __file__]
    for root, _, files in os.walk(os.path.join(HERE, "ref_shim")):
        own += [os.path.join(root, f) for f in files]
    stamp = hashlib.sha256(("".join(sorted(shas.values())) + "".join(_sha(p) for p in sorted(own))
                            + " ".join(CXXFLAGS)).encode()).hexdigest()
    stamp_path = os.path.join(OUT, "stamp")
    if not force and os.path.isfile(LIB) and os.path.isfile(stamp_path) and open(stamp_path).read() == stamp:
        return LIB
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(ref, "APD.cu"), "rb") as f:
        lines = f.read().split(b"\n")
    text_lines = [l.decode("latin-1") for l in lines]
    cut = cut_device_text(text_lines)
    check_table(table, text_lines[:cut])
    with open(os.path.join(OUT, "APD_device.cpp"), "wb") as f:
        f.write(b"\n".join(lines[:cut]) + b"\n")
    shutil.copyfile(os.path.join(ref, "APD.h"), os.path.join(OUT, "APD.h"))
    shutil.copyfile(os.path.join(ref, "main.h"), os.path.join(OUT, "main.h"))
    with open(os.path.join(OUT, "ref_draws.inc"), "w") as f:
        for d in table["draws"]:
            f.write("\t{%d, %d, %d},\n" % (d["first"], d["last"], SUBS[d["sub"]]))
    cxx = os.environ.get("CXX", "g++")
    # -Bsymbolic: the device text's plain names (min, max, threadIdx, ...) bind inside the library whatever else the process holds
    cmd = [cxx] + CXXFLAGS + ["-I" + os.path.join(HERE, "ref_shim"), "-I" + OUT, "-shared", "-Wl,-Bsymbolic", "-o", LIB + ".tmp",
                              os.path.join(OUT, "APD_device.cpp"), os.path.join(HERE, "ref_harness.cpp")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    with open(stamp_path, "w") as f:
        f.write(stamp)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
