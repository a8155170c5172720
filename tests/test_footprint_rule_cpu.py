"""The footprint rule that picks streaming or cache-resident kernel variants (csrc/bk_common.hpp: bk_distinct_arrays,
bk_streams_past_llc), run on the host in a stand-alone program, and its use at the launch sites whose arrays may alias."""
import os
import subprocess

import bayes_kit_amd as bk
from bayes_kit_amd.targets import _find_hipcc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "bayes-kit_amd", "csrc")

PROGRAM = r"""
#include "bk_common.hpp"
#include <stdio.h>
int main() {
  double a[1], b[1], c[1], d[1], e[1];
  int bad = 0;
#define CHECK_EQ(x, want) do { long long g_ = (long long)(x); if (g_ != (want)) { printf("FAIL %s = %lld, want %d\n", #x, g_, (want)); bad = 1; } } while (0)
  CHECK_EQ(bk_distinct_arrays({a, b, c, d, e}), 5);           // out of place
  CHECK_EQ(bk_distinct_arrays({a, a, b, b, c}), 3);           // the in-place step: theta, theta, rho, rho, grad
  CHECK_EQ(bk_distinct_arrays({a, b, c, c, d}), 4);           // the first step of a trajectory: rho in place
  CHECK_EQ(bk_distinct_arrays({a, b, a, b, a}), 2);           // repeats that are not neighbours
  CHECK_EQ(bk_distinct_arrays({a, a, a}), 1);
  CHECK_EQ(bk_distinct_arrays({a, nullptr, b, nullptr}), 2);  // null pointers count nothing
  CHECK_EQ(bk_distinct_arrays({nullptr, nullptr}), 0);
  CHECK_EQ(bk_distinct_arrays({}), 0);
  // 192 MiB itself still fits; D = 1,024: three arrays of 8,192 chains
  CHECK_EQ(bk_streams_past_llc(3 * (i64)8192 * 1024), 0);
  CHECK_EQ(bk_streams_past_llc(3 * (i64)8194 * 1024), 1);
  CHECK_EQ(bk_streams_past_llc(bk_distinct_arrays({a, a, b, b, c}) * (i64)8192 * 1024), 0);  // resident: plain variant
  CHECK_EQ(bk_streams_past_llc(bk_distinct_arrays({a, a, b, b, c}) * (i64)8194 * 1024), 1);
  CHECK_EQ(bk_streams_past_llc(bk_distinct_arrays({a, b, c, c, d}) * (i64)8192 * 1024), 1);  // 256 MiB: streams
  CHECK_EQ(bk_streams_past_llc(bk_distinct_arrays({a, b}) * (i64)12288 * 1024), 0);          // the gradient op's own seam
  CHECK_EQ(bk_streams_past_llc(bk_distinct_arrays({a, b}) * (i64)12290 * 1024), 1);
  if (!bad) printf("ok\n");
  return bad;
}
"""


def test_distinct_arrays_and_threshold_on_the_host(tmp_path):
    src, exe = tmp_path / "footprint.cpp", tmp_path / "footprint"
    src.write_text(PROGRAM)
    # host side only: the program calls nothing of HIP, so it needs no GPU to run
    r = subprocess.run([_find_hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_launch_sites_count_different_arrays():
    assert "bk_streams_past_llc(arrays * C * D)" in _read("bk_integrator.hip")
    assert "arrays = bk_distinct_arrays({theta_in, theta_out, rho_in, rho_out, grad})" in _read("bk_integrator.hip")
    assert "bk_streams_past_llc(bk_distinct_arrays({theta, grad}) * C * D)" in _read("bk_targets.hip")
    assert "bk_streams_past_llc(bk_distinct_arrays({theta, rho}) * n * D)" in _read("bk_elementwise.hpp")
    assert "bk_streams_past_llc(bk_distinct_arrays({work, out, loc_in}) * C * D)" in _read("bk_rng.hip")


def test_the_samplers_threshold_is_the_librarys():
    """HMCDiag sizes its default tile with LLC_BYTES; the kernels decide with bk_streams_past_llc: the same number."""
    assert "static inline bool bk_streams_past_llc(i64 elems) { return elems * 8 > ((i64)192 << 20); }" in _read("bk_common.hpp")
    assert bk.HMCDiag.LLC_BYTES == 192 << 20
