"""The split strong update at 17 ... 31 source views (DVP_STRONG_WIDE=1: dvp_strong_decide_wide, strong_decide_wide_px), against
the oracle bit for bit after every launch of a FIRST_INIT and a REFINE_ITER pass — the cases of tests/test_view_counts.py, whose
helpers and oracle runs are shared, with the switch set before the engine is made.

S = 17: one view in the fifth 16-byte piece; 20: five whole pieces (the count the reference's converter writes); 21; 28: seven
whole pieces; 31: the C ABI's maximum, whose last piece reads one word past the last record.  Full masks at S = 20 / 31 are the
reference's limit of 19 source directions in GenerateRandomNormal_YZL with 20 / 31 bits set.

CPU: host emulation — strong_decide_px<16> hands S > 16 to strong_decide_wide_px in host builds.  The emulation cannot reach the
streaming text at S <= 16 (DVP_STRONG_WIDE=2) without a change to tests/emul/emul.cpp, whose dispatch takes a bracket of 32 to
strong_decide_px<16>, which holds S <= 16 itself: those counts run on the GPU only.
GPU (-m gpu): the HIP library through the C ABI, with dvp_strong_update_form saying which decision kernel ran."""
import pytest

from conftest import first_pass_state, stage_sequence
from test_view_counts import view_count_case, full_masks_case, emul_engine, gpu_engine, make_scene, pass_params, FORMS

DEFAULT_S = [17, 20, 21, 28, 31]
LOCKSTEP_S = [17, 20, 31]
assert "default" in FORMS and "strong_split_lockstep_refine" in FORMS


def wide(monkeypatch, value="1"):
    monkeypatch.setenv("DVP_STRONG_WIDE", value)


def checked_gpu_engine(want):
    """gpu_engine whose contexts report `want` when they are made (the answer then assumes that the cost buffers fit); the
    callers ask the contexts again after the case has run"""
    made = []

    def make(sc, p, depths):
        g = gpu_engine(sc, p, depths)
        assert g.strong_update_form() == want, (g.strong_update_form(), want)
        made.append(g)
        return g
    return make, made


def form_after_the_first_strong_update(S):
    sc = make_scene(S)
    g = gpu_engine(sc, pass_params(S)[0], None)
    g.upload_state(**first_pass_state(sc))
    for stg, it, col in stage_sequence(1):
        g.run_stage(stg, it, col)
        if stg == "strong_update":
            break
    form = g.strong_update_form()
    g.close()
    return form


@pytest.mark.parametrize("S", DEFAULT_S)
def test_wide_default_form_emulated_kernels(S, monkeypatch):
    wide(monkeypatch)
    view_count_case(S, "default", emul_engine, monkeypatch)


@pytest.mark.parametrize("S", LOCKSTEP_S)
def test_wide_lockstep_refine_emulated_kernels(S, monkeypatch):
    wide(monkeypatch)
    view_count_case(S, "strong_split_lockstep_refine", emul_engine, monkeypatch)


def test_wide_without_the_plane_cache_emulated_kernels(monkeypatch):
    wide(monkeypatch)
    monkeypatch.setenv("DVP_STRONG_REUSE", "0")
    view_count_case(20, "default", emul_engine, monkeypatch)


def test_wide_half_planes_emulated_kernels(monkeypatch):
    wide(monkeypatch)
    view_count_case(20, "default", emul_engine, monkeypatch, "box")


@pytest.mark.parametrize("S", [20, 31])
def test_wide_full_masks_emulated_kernels(S, monkeypatch):
    wide(monkeypatch)
    full_masks_case(S, emul_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("S", DEFAULT_S)
def test_wide_default_form_gpu(S, monkeypatch):
    wide(monkeypatch)
    make, made = checked_gpu_engine(32)
    view_count_case(S, "default", make, monkeypatch)
    assert len(made) == 2 and all(g.strong_update_form() == 32 for g in made)


@pytest.mark.gpu
@pytest.mark.parametrize("S", LOCKSTEP_S)
def test_wide_lockstep_refine_gpu(S, monkeypatch):
    wide(monkeypatch)
    make, made = checked_gpu_engine(32)
    view_count_case(S, "strong_split_lockstep_refine", make, monkeypatch)
    assert len(made) == 2 and all(g.strong_update_form() == 32 for g in made)


@pytest.mark.gpu
def test_wide_without_the_plane_cache_gpu(monkeypatch):
    wide(monkeypatch)
    monkeypatch.setenv("DVP_STRONG_REUSE", "0")
    make, made = checked_gpu_engine(32)
    view_count_case(20, "default", make, monkeypatch)
    assert len(made) == 2 and all(g.strong_update_form() == 32 for g in made)


@pytest.mark.gpu
def test_wide_half_planes_gpu(monkeypatch):
    wide(monkeypatch)
    make, made = checked_gpu_engine(32)
    view_count_case(20, "default", make, monkeypatch, "box")
    assert len(made) == 2 and all(g.strong_update_form() == 32 for g in made)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [20, 31])
def test_wide_full_masks_gpu(S, monkeypatch):
    wide(monkeypatch)
    make, made = checked_gpu_engine(32)
    full_masks_case(S, make)
    assert len(made) == 1 and made[0].strong_update_form() == 32


@pytest.mark.gpu
def test_strong_update_form_follows_the_switch(monkeypatch):
    """S = 17: 32 with the switch, 0 (the monolithic kernel) without it; S <= 16: the brackets, 32 under DVP_STRONG_WIDE=2"""
    for value, S, want in ((None, 17, 0), ("0", 17, 0), ("1", 17, 32), ("2", 17, 32), (None, 9, 10), ("1", 16, 16), ("2", 9, 32)):
        if value is None:
            monkeypatch.delenv("DVP_STRONG_WIDE", raising=False)
        else:
            wide(monkeypatch, value)
        assert form_after_the_first_strong_update(S) == want, (value, S)


@pytest.mark.gpu
def test_no_room_for_the_cost_buffer_is_monolithic(monkeypatch):
    """DVP_TEST_SPLIT_ALLOC_FAIL: the cost buffer's allocation reports failure — the context says 0 once its first strong update has
    tried, and still equals the oracle"""
    wide(monkeypatch)
    monkeypatch.setenv("DVP_TEST_SPLIT_ALLOC_FAIL", "1")
    made = []

    def make(sc, p, depths):
        made.append(gpu_engine(sc, p, depths))
        return made[-1]
    view_count_case(17, "default", make, monkeypatch)
    assert len(made) == 2 and all(g.strong_update_form() == 0 for g in made)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 4, 5, 9, 12, 16])
def test_wide_at_every_bracket_gpu(S, monkeypatch):
    """DVP_STRONG_WIDE=2: the streaming kernel in place of dvp_strong_decide_v4 ... v16"""
    wide(monkeypatch, "2")
    make, made = checked_gpu_engine(32)
    view_count_case(S, "default", make, monkeypatch)
    assert len(made) == 2 and all(g.strong_update_form() == 32 for g in made)
