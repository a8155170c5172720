"""CTarget.from_source(form="lanes", neighbour=True) on the build box (hipcc only, no compute): neighbour sources compile for
every head and row count, export what include/bkhip_source.h lists, the flag is refused by the other forms, the pair calls do
not compile without it, and the generated text of existing lanes sources is what it was before the flag existed."""
import ctypes
import hashlib

import pytest

import bayes_kit_amd as bk
from bayes_kit_amd import targets as T
from tests.helpers import cache_tmp_path  # noqa: F401  (fixture)
from tests.neighbour_models import SSM_SRC, ar1_src
from tests.test_from_source_cpu import CHAIN, LANES, TERM
from tests.test_gpu_providers import FUNNEL_LANES_SRC, HIER_LANES_SRC

ALL = ("bk_src_target", "bk_src_target_n", "bk_src_leapfrog_step", "bk_src_dr_proposal_job", "bk_src_hmc_trajectory_lanes",
       "bk_src_hmc_trajectory", "bk_src_hmc_draw", "bk_src_mala_step", "bk_src_trajectory")


@pytest.fixture()
def cache(cache_tmp_path, monkeypatch):
    d = cache_tmp_path / "cache"
    monkeypatch.setenv("BK_SOURCE_TARGET_DIR", str(d))
    return d


def exports(lib):
    h = ctypes.CDLL(lib)
    return {n for n in ALL if hasattr(h, n)}


def test_neighbour_sources_compile_and_export_the_lanes_entry_points(cache):
    specs = [dict(user_source=ar1_src(head), form="lanes", contract=False, dims=head + rows, head=head, neighbour=True)
             for head in (0, 1, 2) for rows in (1, 15, 16, 17, 99, 128, 129, 300)]
    errors = []
    assert T.prewarm_sources(specs, errors=errors) == (len(specs), 0), errors
    for sp in specs:
        lib = T._compile_source_target(sp["user_source"], "lanes", False, sp["dims"], sp["head"], neighbour=True)
        rows = sp["dims"] - sp["head"]
        want = {"bk_src_target", "bk_src_target_n"}
        if rows <= 128:  # (bkhip_source.h: the one-launch step, HMC trajectory and proposal kernels)
            want |= {"bk_src_leapfrog_step", "bk_src_hmc_trajectory_lanes", "bk_src_dr_proposal_job"}
        assert exports(lib) == want, (sp["head"], rows)
    # the objects: the hooks the samplers key on follow the exports
    t = bk.CTarget.from_source(ar1_src(2), 101, form="lanes", head=2, neighbour=True)
    assert t.source_neighbour and t.source_form == "lanes"
    assert hasattr(t, "bk_dr_proposal") and hasattr(t, "bk_hmc_proposal") and hasattr(t, "bk_leapfrog_step")
    big = bk.CTarget.from_source(ar1_src(0), 300, form="lanes", head=0, neighbour=True)
    assert not hasattr(big, "bk_dr_proposal") and not hasattr(big, "bk_leapfrog_step") and big.bk_counted
    assert not bk.CTarget.from_source(LANES, 101, form="lanes", head=1).source_neighbour
    ssm = T._compile_source_target(SSM_SRC, "lanes", False, 101, 2, neighbour=True)
    assert "bk_src_dr_proposal_job" in exports(ssm)


def test_neighbour_flag_belongs_to_the_lanes_form(cache):
    for form, src in (("chain", CHAIN), ("elementwise", TERM)):
        with pytest.raises(ValueError, match="neighbour"):
            T._source_text(src, form, 16, 0, neighbour=True)
        with pytest.raises(ValueError, match="neighbour"):
            bk.CTarget.from_source(src, 16, form=form, neighbour=True)


def test_pair_calls_do_not_compile_without_the_flag(cache):
    with pytest.raises(bk._lib.BkHipError, match="neighbour"):
        T._compile_source_target(ar1_src(1), "lanes", False, 40, 1)
    # a spec without the key (a manifest line written before the flag existed) builds without it: the same failure
    specs = [dict(user_source=ar1_src(1), form="lanes", contract=False, dims=40, head=1, stage="auto")]
    assert T.prewarm_sources(specs) == (0, 1)
    assert T.prewarm_sources([dict(specs[0], neighbour=True)]) == (1, 0)


def test_existing_sources_generate_the_same_text(cache, monkeypatch, tmp_path):
    """The generated translation unit of a source without the flag is byte for byte what it was before neighbour= existed
    (sha256 taken from the tree before the change): same text, same cache key, same library."""
    pinned = {
        ("funnel", 101, 1): "eec9f857f419b331a852c3d8a058aa8d7908e7b5d7bd6feda276517fd4aa11e3",
        ("funnel", 300, 1): "04564c088b89b7700f99e4a52b06986242b27e7bd546ec7b9e209e7fcb1f0908",
        ("funnel", 17, 1): "f7b38bc309aa7841d28b1cce07f6e9cd43e07661091da46884b6c8be49435f82",
        ("hier", 52, 2): "e214d228472763b21cea152bad8d797a652214c52ffa6910e3be3be265dcd9db",
        ("hier", 130, 2): "454671bb1ade31da3ae5edff3500cda0929dbfcc1e4fc0ae80bb495a7981adec",
        ("lanes", 101, 1): "2a2727868f0c99c1feb72bd7961e0c0eb07449ccecb94134f334f4a8d398ec60",
    }
    srcs = {"funnel": FUNNEL_LANES_SRC, "hier": HIER_LANES_SRC, "lanes": LANES}
    for (name, D, head), want in pinned.items():
        for kw in ({}, {"neighbour": False}):
            text = T._source_text(srcs[name], "lanes", D, head, **kw)
            assert hashlib.sha256(text.encode()).hexdigest() == want, (name, D, head)
    assert T._source_text(ar1_src(1), "lanes", 40, 1, neighbour=True).count("#define BK_SOURCE_NEIGHBOUR 1\n") == 1
    # the request log: the flag only where it is set
    import json

    rec = tmp_path / "rec.jsonl"
    monkeypatch.setenv("BK_SOURCE_RECORD", str(rec))
    T._compile_source_target(LANES, "lanes", False, 101, 1)
    T._compile_source_target(ar1_src(1), "lanes", False, 40, 1, neighbour=True)
    asked = [json.loads(line) for line in open(rec)]
    assert "neighbour" not in asked[0] and asked[1]["neighbour"] is True
