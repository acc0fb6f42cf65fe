"""The XCD-aware tile orders (numpy-quant_amd/csrc/nqk_xcd.h: xcd_remap of k_embed_q /
k_embed_q16 / k_qgemm_big, xcd_walk of the persistent k_pg) are permutations of the tile ids
for EVERY XCD count, not only the MI355X's 8: a host program around the header checks XC in
1..16 and 1..600 tiles (and, for the walk, grids from one workgroup to more than tiles).
ADVICE r6: k_embed_q computed its band index as b / 8 while the bands used the device's XCD
count — on any other count some tiles ran several times and others never."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "nqk_xcd.h"
int main() {
  long bad = 0;
  for (int xc = 1; xc <= 16; ++xc)
    for (int t = 1; t <= 600; ++t) {
      std::vector<int> seen(t, 0);
      for (int b = 0; b < t; ++b) {
        const long tile = nqk::xcd_remap<long>(b, t, xc);
        const int tile32 = nqk::xcd_remap<int>(b, t, xc);
        if (tile < 0 || tile >= t || tile32 != tile) { ++bad; continue; }
        ++seen[tile];
      }
      for (int i = 0; i < t; ++i) bad += seen[i] != 1;
      // the persistent walk: grids of 1, a few, t - 1, t, and more workgroups than tiles
      const int grids[] = {1, 2, 3, 7, 8, 16, 37, 256, 512, t > 1 ? t - 1 : 1, t, t + 5};
      for (int g : grids) {
        if (g > t) continue;  // the launcher never starts more workgroups than tiles
        std::vector<int> hit(t, 0);
        for (int b = 0; b < g; ++b) {
          const nqk::XcdWalk w = nqk::xcd_walk(b, g, t, xc);
          if (w.iters < 0 || w.step < 1) { ++bad; continue; }
          for (int it = 0; it < w.iters; ++it) {
            const int tile = w.first + it * w.step;
            if (tile < 0 || tile >= t) ++bad; else ++hit[tile];
          }
        }
        for (int i = 0; i < t; ++i) bad += hit[i] != 1;
      }
    }
  // the parent's k_embed_q form (b / 8 for the band position) is NOT a permutation at XC = 4
  {
    const int xc = 4, t = 24;
    std::vector<int> seen(t, 0);
    for (int b = 0; b < t; ++b) {
      const int x = b % xc, q = t / xc, r = t % xc, tile = x * q + (x < r ? x : r) + b / 8;
      if (tile >= 0 && tile < t) ++seen[tile];
    }
    int once = 0;
    for (int i = 0; i < t; ++i) once += seen[i] == 1;
    if (once == t) ++bad;  // the check itself would be blind
  }
  std::printf("bad=%ld\n", bad);
  return bad != 0;
}
"""


def test_xcd_tile_orders_are_permutations(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "xcd_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "xcd_check"
    inc = os.path.join(ROOT, "numpy-quant_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", inc, str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "bad=0", res.stdout + res.stderr
