"""The per-view (pixel, view) lists of the sweep passes' evaluation launches (csrc/dvp_sweep_list.hpp) without a GPU:
tests/sweep_list_host builds the list functions the kernels share with the host — count per (view, tile), scan, ballot-rank fill —
into a stand-alone program under the address and undefined-behaviour sanitizers.  Its lists are compared here with a direct numpy
enumeration of sweep_go in the order rule: tiles (64 x 14) in the strip order of the evaluation launch — strips of 8 tile columns,
row-major inside a strip —, rows inside a tile top to bottom, x ascending inside a row.  The program itself checks that the
workgroups of an evaluation launch take every entry exactly once for R = 2, 4, 8 and 16."""
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sweep_list_host")
VALID, REFINE, PEAK = 1, 2, 4      # dvp_sweep.hpp: SWF_*
ROWS = 14                          # dvp_forms.hpp: kSweepRows


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", _HERE, "sweep_list_host"])
    return os.path.join(_HERE, "sweep_list_host")


def run(exe, tmp_path, W, H, S, stage, flags, sel, vw):
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "lists.bin")
    with open(case, "wb") as f:
        np.array([W, H, S, stage], np.int32).tofile(f)
        flags.astype(np.int32).tofile(f)
        sel.astype(np.uint32).tofile(f)
        vw.astype(np.uint8).tofile(f)
    r = subprocess.run([exe, case, res], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("checks ok"), r.stdout + r.stderr
    out = np.fromfile(res, np.uint32)
    R, S_ = int(out[0]), int(out[1])
    assert S_ == S
    n = out[2:2 + S].astype(np.int64)
    lists, at = [], 2 + S
    for v in range(S):
        lists.append(out[at:at + n[v]])
        at += int(n[v])
    assert at == out.size
    return R, lists


def go(W, H, S, stage, flags, sel, vw):
    """sweep_go for every (pixel, view): [H, W, S]"""
    need = VALID if stage == 0 else PEAK
    bits = (sel[:, None] >> np.arange(S, dtype=np.uint32)[None, :]) & 1
    return (((flags & need) != 0)[:, None] & (bits == 1) & (vw[:, :S] != 0)).reshape(H, W, S)


def tile_order(W, H):
    tiles_x, tiles_y = (W + 63) // 64, (H + ROWS - 1) // ROWS
    for st in range(0, tiles_x, 8):
        for ty in range(tiles_y):
            for tx in range(st, min(st + 8, tiles_x)):
                yield tx, ty


def expected(W, H, S, g):
    want = [[] for _ in range(S)]
    for tx, ty in tile_order(W, H):
        for y in range(ty * ROWS, min((ty + 1) * ROWS, H)):
            for x in range(tx * 64, min((tx + 1) * 64, W)):
                for v in np.nonzero(g[y, x])[0]:
                    want[v].append((y << 16) | x)
    return [np.array(w, np.uint32) for w in want]


def state(W, H, S, seed):
    rng = np.random.default_rng(seed)
    L = W * H
    flags = np.where(rng.random(L) < 0.9, VALID, 0)
    flags = np.where((flags != 0) & (rng.random(L) < 0.8), flags | REFINE, flags)
    flags = np.where((flags != 0) & (rng.random(L) < 0.6), flags | PEAK, flags)   # what a decide1 leaves: some valid pixels without a central peak
    yy, xx = np.divmod(np.arange(L), W)
    flags[(xx < 6) | (yy < 6) | (xx >= W - 6) | (yy >= H - 6)] = 0                 # the frame is not the passes'
    sel = rng.integers(0, 1 << S, L).astype(np.uint32)
    sel |= rng.integers(0, 1 << 32, L, dtype=np.uint64).astype(np.uint32) & np.uint32((0xFFFFFFFF << S) & 0xFFFFFFFF)   # bits of views that do not exist
    vw = rng.integers(1, 256, (L, 32)).astype(np.uint8)
    vw[rng.random((L, 32)) < 0.2] = 0
    return flags, sel, vw


def check(exe, tmp_path, W, H, S, stage, flags, sel, vw):
    R, lists = run(exe, tmp_path, W, H, S, stage, flags, sel, vw)
    want = expected(W, H, S, go(W, H, S, stage, flags, sel, vw))
    for v in range(S):
        assert lists[v].size == want[v].size, v
        assert (lists[v] == want[v]).all(), v
    return R, lists


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("W,H,S", [(96, 64, 9), (96, 64, 1), (40, 30, 1), (40, 30, 2), (40, 30, 9), (600, 30, 3)])
def test_lists_equal_the_enumeration(exe, tmp_path, W, H, S, stage):
    """96 x 64: the second tile column is 32 wide, the last tile row 8 high; 40 x 30: narrower than a tile; 600 x 30: ten tile
    columns, i.e. a full strip and a ragged one.  Stage 1 takes the pixels whose flags a decide1 marked with a central peak."""
    flags, sel, vw = state(W, H, S, 11 * W + S)
    R, lists = check(exe, tmp_path, W, H, S, stage, flags, sel, vw)
    assert sum(l.size for l in lists) > 0
    if stage == 1:
        R0, lists0 = run(exe, tmp_path, W, H, S, 0, flags, sel, vw)
        assert all(l1.size < l0.size or l0.size == 0 for l0, l1 in zip(lists0, lists))


def test_empty_lists(exe, tmp_path):
    """view 3: no pixel selects it; view 5: selected everywhere, weight 0 everywhere"""
    W, H, S = 96, 64, 9
    flags, sel, vw = state(W, H, S, 5)
    sel &= ~np.uint32(1 << 3)
    sel |= np.uint32(1 << 5)
    vw[:, 5] = 0
    R, lists = check(exe, tmp_path, W, H, S, 0, flags, sel, vw)
    assert lists[3].size == 0 and lists[5].size == 0
    assert all(lists[v].size > 0 for v in (0, 1, 2, 4, 6, 7, 8))
    # ... and nothing takes part at all
    R, lists = check(exe, tmp_path, W, H, S, 1, flags & ~PEAK, sel, vw)
    assert all(l.size == 0 for l in lists)


def test_list_lengths_around_a_workgroups_share(exe, tmp_path):
    """lists of 0, 1, 64 R - 1, 64 R and 64 R + 1 entries (R rounds of 64 per workgroup)"""
    W, H, S = 96, 64, 9
    flags, sel, vw = state(W, H, S, 3)
    R, _ = run(exe, tmp_path, W, H, S, 0, flags, sel, vw)
    rng = np.random.default_rng(17)
    inner = np.nonzero(flags & VALID)[0]
    lengths = [0, 1, 64 * R - 1, 64 * R, 64 * R + 1]
    assert lengths[-1] <= inner.size
    vw[:, :5] = 9
    sel &= ~np.uint32(31)
    for v, n in enumerate(lengths):
        sel[rng.choice(inner, n, replace=False)] |= np.uint32(1 << v)
    R, lists = check(exe, tmp_path, W, H, S, 0, flags, sel, vw)
    assert [lists[v].size for v in range(5)] == lengths
