"""The driver's host-only pieces without a GPU, through tests/host/test_host: the host visibility clean-up
(CleanSelectedViewsOnHost: what `apd --cleanup-on host` runs and what the device clean-up is defined against) on every case of
np_viewclean.cases() against scipy's components, the command line (ParseOptions) and the pass list (BuildPlan + ConfigurePass)
against tables written out here."""
import os
import re
import subprocess

import numpy as np
import pytest

import np_viewclean as V
from conftest import ROOT

pytestmark = pytest.mark.hostbox

TEST_HOST = os.path.join(ROOT, "tests", "host", "test_host")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])


def _run(*args, env=None):
    return subprocess.run([TEST_HOST] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)


# ---- clean-up ----------------------------------------------------------------------------------------------------------------------
# Every case of np_viewclean.cases(): the host loop takes every source count they use (0, 1, 3, 9, 31 and 32 — one bit of the word
# per source), so none is left out.
@pytest.mark.parametrize("name", sorted(V.cases()))
def test_host_cleanup_equals_scipy(tmp_path, name):
    views, num_src, min_region = V.cases()[name]
    H, W = views.shape
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(views, np.uint32).tofile(src)
    r = _run("--cleanup", src, W, H, num_src, min_region, out)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, np.uint32).reshape(H, W)
    want = V.np_clean(views, num_src, min_region)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


# ---- options -----------------------------------------------------------------------------------------------------------------------
def _options(*args, env=None):
    r = _run("--options", "/data/scene", *args, env=env)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("DVP_JOB_ID", "TORCHELASTIC_RUN_ID", "SLURM_JOB_ID")}
    env.update(extra)
    return env


DEFAULTS = dict(dense_folder="/data/scene", gpu="0", max_src="0", iters="3", min_scale="2", geom_passes="3", rank="0", world="1", seed="1234", fusion="1", jacobi="0",
                collective_timeout_s="600", sync_io="0", host_rescale="0", previews="0", views_in_flight="0", in_flight_pixels=str(2 << 20), job="", transport="rccl",
                fusion_on_host="0", fusion_kind="eth", use_label_files="0", edges_on_device="0", cleanup_on_device="0", labels_on_device="0", prior_on_device="0",
                images_on_device="0", decode_on_device="0", device_rescale="1", device_maps="1", strong_wide="0", final_iteration="15")

# option of the usage string -> (its arguments, the fields it changes)
USAGE_OPTIONS = {
    "--previews": ([], dict(previews="1")),
    "--max-src": (["7"], dict(max_src="7")),
    "--iters": (["5"], dict(iters="5")),
    "--min-scale": (["1"], dict(min_scale="1")),
    "--passes": (["2"], dict(geom_passes="2")),
    "--seed": (["1844674407370955161"], dict(seed="1844674407370955161")),
    "--rank": (["1"], dict(rank="1")),
    "--world": (["2"], dict(world="2", jacobi="1")),
    "--job": (["run-17"], dict(job="run-17")),
    "--jacobi": ([], dict(jacobi="1")),
    "--no-fusion": ([], dict(fusion="0")),
    "--fusion": (["tat-advanced"], dict(fusion_kind="tat-advanced")),
    "--fusion-on": (["host"], dict(fusion_on_host="1")),
    "--edges-on": (["gpu"], dict(edges_on_device="1")),
    "--labels-on": (["gpu"], dict(labels_on_device="1")),
    "--cleanup-on": (["gpu"], dict(cleanup_on_device="1")),
    "--images-on": (["gpu"], dict(images_on_device="1")),
    "--prior-on": (["gpu"], dict(prior_on_device="1")),
    "--decode-on": (["gpu"], dict(decode_on_device="1")),
    "--strong-wide": (["on"], dict(strong_wide="1")),
    "--views-in-flight": (["3"], dict(views_in_flight="3")),
}
# ... and the options ParseOptions takes beyond it
OTHER_OPTIONS = {
    "--labels": ([], dict(use_label_files="1")),
    "--sync-io": ([], dict(sync_io="1", device_rescale="0", device_maps="0")),
    "--host-rescale": ([], dict(host_rescale="1", device_rescale="0", device_maps="0")),
    "--transport": (["host"], dict(transport="host")),
    "--collective-timeout": (["30"], dict(collective_timeout_s="30")),
    "--in-flight-pixels": (["1000"], dict(in_flight_pixels="1000")),
}
CHOICES = {"--edges-on": "host or gpu", "--labels-on": "host or gpu", "--cleanup-on": "host or gpu", "--images-on": "host or gpu", "--prior-on": "host or gpu",
           "--decode-on": "host or gpu", "--strong-wide": "on or off"}


def test_defaults_are_a_default_run_config():
    assert _options(env=_clean_env()) == DEFAULTS


def test_the_table_has_every_option_of_the_usage_string():
    r = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stderr.startswith("USAGE: apd dense_folder [gpu_index]")
    assert set(re.findall(r"--[a-z-]+", r.stderr)) == set(USAGE_OPTIONS)


@pytest.mark.parametrize("option", sorted(USAGE_OPTIONS) + sorted(OTHER_OPTIONS))
def test_option_sets_its_fields_and_nothing_else(option):
    args, changed = {**USAGE_OPTIONS, **OTHER_OPTIONS}[option]
    assert all(DEFAULTS[k] != v for k, v in changed.items())
    assert _options(option, *args, env=_clean_env()) == dict(DEFAULTS, **changed)


def test_all_options_together_with_the_gpu_index():
    args, want = ["3"], dict(DEFAULTS, gpu="3")
    for option, (a, changed) in {**USAGE_OPTIONS, **OTHER_OPTIONS}.items():
        args += [option] + a
        want.update(changed)
    assert _options(*args, env=_clean_env()) == want


def test_gpu_index_present_and_absent():
    assert _options("5", "--iters", "4", env=_clean_env()) == dict(DEFAULTS, gpu="5", iters="4")
    assert _options("--iters", "4", env=_clean_env()) == dict(DEFAULTS, iters="4")     # an option in its place: device 0


@pytest.mark.parametrize("option", sorted(CHOICES))
def test_choice_option_refuses_another_word(option):
    for word in ("maybe", "GPU", "On", ""):
        r = _run("--options", "/data/scene", option, word)
        assert r.returncode != 0 and r.stdout == ""
        assert r.stderr == "%s takes %s\n" % (option, CHOICES[option])
    first, second = CHOICES[option].split(" or ")
    for word in (first, second):
        assert _run("--options", "/data/scene", option, word).returncode == 0


def test_the_grammars_oddities_stay():
    env = _clean_env()
    assert _options("--no-such-option", "--iters", "4", "--another", env=env) == dict(DEFAULTS, iters="4")     # unknown options are ignored
    assert _options("--seed", "9", "--iters", env=env) == dict(DEFAULTS, seed="9", iters="0")                  # a value option at the end reads as 0
    assert _options("--iters", "4", "--edges-on", env=env) == dict(DEFAULTS, iters="4")                        # a choice option at the end is ignored
    assert _options("--views-in-flight", "99", env=env)["views_in_flight"] == "4"                              # clamped to the context pool's slots
    assert _options("--fusion-on", "elsewhere", env=env) == DEFAULTS                                           # anything but `host` is the device


def test_world_implies_jacobi():
    assert _options("--world", "2", env=_clean_env())["jacobi"] == "1"
    assert _options("--world", "1", env=_clean_env())["jacobi"] == "0"


def test_job_falls_back_to_the_launchers_id():
    assert _options(env=_clean_env(DVP_JOB_ID="from-env"))["job"] == "from-env"
    assert _options(env=_clean_env(SLURM_JOB_ID="s", TORCHELASTIC_RUN_ID="t"))["job"] == "t"
    assert _options(env=_clean_env(SLURM_JOB_ID="s", TORCHELASTIC_RUN_ID="t", DVP_JOB_ID="d"))["job"] == "d"
    assert _options("--job", "mine", env=_clean_env(DVP_JOB_ID="from-env"))["job"] == "mine"


# ---- plan --------------------------------------------------------------------------------------------------------------------------
# The reference's loop (main.cpp:448-512), restated by hand.  Per pass: level, scale, geom_index (-1 = the A pass), state (0 FIRST_INIT,
# 1 REFINE_INIT, 2 REFINE_ITER), use_APD, use_detail, geom_consistency, weak_peak_radius, rotate_time, ransac_threshold; the pass'
# index in the list is its `iteration`.  A Problem's params are carried from pass to pass: use_detail, which only a REFINE_INIT pass
# sets, stays for the level's REFINE_ITER passes; the first pass keeps PatchMatchParams' defaults (rotate_time 4, threshold 0.005).
def _level(level, scale, passes, detail, rotate, ransac):
    first = (level, scale, -1, 0, 0, 0, 0, 6, 4, "0.00500") if level == 0 else (level, scale, -1, 1, 1, detail, 0, 6, rotate, ransac)
    return [first] + [(level, scale, j, 2, int(level != 0), detail, 1, (4, 2, 2)[j], rotate, ransac) for j in range(passes)]


PLANS = {
    # the reference's rule `i < round_num - 1` on a four-level pyramid: three levels, scales 8, 4, 2 (12 passes, last index 11)
    (4, 2, 3): _level(0, 8, 3, 0, 1, "0.01000") + _level(1, 4, 3, 1, 2, "0.00875") + _level(2, 2, 3, 1, 4, "0.00750"),
    # the reference's default schedule of 4 levels x (1 + 3) passes, the one whose last index is the literal 15 of main.cpp:378, is
    # the one of a FIVE-level pyramid
    (5, 2, 3): _level(0, 16, 3, 0, 1, "0.01000") + _level(1, 8, 3, 1, 2, "0.00875") + _level(2, 4, 3, 1, 4, "0.00750") + _level(3, 2, 3, 1, 4, "0.00625"),
    # --min-scale 1 adds the finest level, where the reference's own rule leaves use_detail off
    (2, 1, 1): _level(0, 2, 1, 0, 1, "0.01000") + _level(1, 1, 1, 0, 2, "0.00875"),
    # a single-level pyramid always runs; no geometric pass
    (1, 2, 0): _level(0, 1, 0, 0, 1, "0.01000"),
}


@pytest.mark.parametrize("key", sorted(PLANS))
def test_plan_and_pass_configuration(key):
    r = _run("--plan", *key)
    assert r.returncode == 0, r.stderr
    got = []
    for it, line in enumerate(r.stdout.splitlines()):
        head, fields = line.split(" | ")
        f = dict(zip(fields.split()[0::2], fields.split()[1::2]))
        level, scale, geom_index = (int(x) for x in head.split())
        assert int(f["iteration"]) == it and int(f["scale_size"]) == scale and f["max_iterations"] == "3"
        got.append((level, scale, geom_index, int(f["state"]), int(f["use_APD"]), int(f["use_detail"]), int(f["geom_consistency"]), int(f["weak_peak_radius"]),
                    int(f["rotate_time"]), f["ransac_threshold"]))
    assert got == PLANS[key]


def test_last_index_of_the_reference_schedule_is_15():
    """ISSUE: "(4, 2, 3), the reference schedule.  Its last index must be 15."  With round_num = 4 the reference's loop
    (`i < round_num - 1`) and BuildPlan both give 3 levels = 12 passes, last index 11 (asserted above); the schedule of 4 levels whose
    last index is 15 belongs to round_num = 5.  Both are held here."""
    assert len(PLANS[(4, 2, 3)]) - 1 == 11 and len(PLANS[(5, 2, 3)]) - 1 == 15
    assert len(_run("--plan", 5, 2, 3).stdout.splitlines()) - 1 == 15 == int(DEFAULTS["final_iteration"])
