"""CPU checks of what the context-free entry points (include/egr_raytracer.h: CONTEXT-FREE FUNCTIONS) promise about their errors: one string per module - a
failure in one module never shows in another's egr_<module>_last_error() -, one string for the four evaluation functions, and one string per thread. Every
call here fails its validation, which runs before any HIP call, so none of this needs a device."""
import importlib
import threading

import pytest

pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def prune_gather_without_arrays(L):
    return L.egr_prune_gather(0, None, 0, 0, None, 0, None)  # num_arrays = 0


def grow_sample_without_output(L):
    return L.egr_grow_sample(0, 0, 1, 0, 1.0, 3.0, None, None)  # out_points = NULL


def test_a_module_reports_only_its_own_failures(L):
    assert prune_gather_without_arrays(L) != 0
    prune = L.egr_prune_last_error().decode()
    assert prune == "libegr_hip: egr_prune_gather: 1..EGR_MAX_PRUNE_ARRAYS table entries are required"
    assert grow_sample_without_output(L) != 0
    grow = L.egr_grow_last_error().decode()
    assert grow == "libegr_hip: egr_grow_sample: out_points is a required output"
    assert L.egr_prune_last_error().decode() == prune  # the grow failure did not reach the prune module's string ...
    assert prune_gather_without_arrays(L) != 0
    assert L.egr_grow_last_error().decode() == grow  # ... nor the other way round
    for other in ("egr_edit_last_error", "egr_eval_last_error", "egr_voxel_last_error", "egr_viewset_last_error"):
        text = getattr(L, other)().decode()
        assert "egr_prune" not in text and "egr_grow" not in text, (other, text)


def test_one_string_speaks_for_the_four_evaluation_functions(L, cabi):
    calls = {"egr_eval_metrics": lambda: L.egr_eval_metrics(0, 0, 1, 1, None, None, None, None, None, None, None, None, None, None),  # num_views = 0
             "egr_eval_ssim": lambda: L.egr_eval_ssim(0, 0, 1, 1, None, None, None, None, None, None, None, None, None),
             "egr_ssim_images": lambda: L.egr_ssim_images(0, 0, 1, 1, None, None, None, None, None, None)}
    for name, call in calls.items():
        assert call() != 0
        assert L.egr_eval_last_error().decode() == "libegr_hip: %s: num_views must be in 1..65535" % name
    assert L.egr_eval_frames(0, None, None) != 0  # args = NULL
    assert L.egr_eval_last_error().decode() == "libegr_hip: egr_eval_frames: args is required"
    assert calls["egr_eval_ssim"]() != 0  # and back: the frames failure is replaced, not kept beside it
    assert L.egr_eval_last_error().decode() == "libegr_hip: egr_eval_ssim: num_views must be in 1..65535"


def test_a_failure_in_another_thread_is_not_visible_here(L):
    assert grow_sample_without_output(L) != 0
    mine = L.egr_grow_last_error().decode()
    seen = {}

    def other():
        seen["before"] = L.egr_grow_last_error().decode()  # a thread that has not failed yet has no message
        seen["rc"] = L.egr_grow_sample(0, 0, 1, 0, -1.0, 3.0, 0x100000, None)  # a negative radius
        seen["after"] = L.egr_grow_last_error().decode()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["before"] == "" and seen["rc"] != 0
    assert seen["after"] == "libegr_hip: egr_grow_sample: radius must be finite and not negative"
    assert L.egr_grow_last_error().decode() == mine == "libegr_hip: egr_grow_sample: out_points is a required output"
