"""The lane map of the staging copy (volume_renderer_amd/csrc/vr_stage_map.h: stage_width, stage_map,
stage_lane, stage_passes, stage_next -- the functions vr_stage.h stage_box calls) simulated on the host:
a stand-alone program built with g++ (once plain, once with the address and undefined-behaviour
sanitizers, run directly) moves every box with 1 <= ex <= 64 and ex * ey * ez <= 2560 (the largest
slot) through the 64 lanes' passes, for 1, 2 and 4 floats per lane, from a source buffer of exactly
the box's rows into a slot buffer of exactly the box's size."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volume_renderer_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "vr_stage_map.h"

static long bad = 0, boxes = 0, moved = 0;
static const vr::UdivTab tab = vr::make_udiv_tab();

template <int V>
static void run_box(uint32_t ex, uint32_t ey, uint32_t ez) {
  const uint32_t rows = ey * ez, vol = ex * rows;
  // exactly the box's rows / the slot's words: a float read or written outside is the sanitizer's
  float *src = new float[vol], *slot = new float[vol];
  std::vector<int> writes(vol, 0);
  for (uint32_t i = 0; i < vol; ++i) {
    src[i] = (float)(i + 1);
    slot[i] = -1.f;
  }
  const vr::StageMap M = vr::stage_map<V>(ex, ey, tab);
  const uint32_t gx = (ex + V - 1) / V, per = 64u / gx, passes = (rows + per - 1) / per;
  if (M.gx != gx || M.per != per || vr::stage_passes(M, rows) != passes) ++bad;
  if (M.wq != per / ey || M.wr != per % ey) ++bad;
  // dense source and slot: the pitches are the box's (a plane step adds nothing on top of its rows)
  const vr::StageStep<uint32_t> S = vr::stage_step<uint32_t>(M, ex, ex * ey, 1u, (int32_t)ex, (int32_t)(ex * ey));
  // a second cursor that only keeps the books: rows advanced in the low word, plane steps in the high
  const vr::StageStep<uint64_t> T = vr::stage_step<uint64_t>(M, 1ull, (1ull << 32) + ey, 1ull, 0, 0);
  uint32_t most = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const vr::StageLane s = vr::stage_lane<V>(M, lane, rows);
    const uint32_t rr = lane / gx, xg = lane % gx;
    const uint32_t x = (xg + 1) * V <= ex ? xg * V : ex - V;
    const uint32_t n = rr < per && rr < rows ? (rows - rr + per - 1) / per : 0;
    if (s.x != x || s.x + V > ex) ++bad;  // the lane's V floats lie in [0, ex) of its row
    if (s.n != n) ++bad;
    if (s.n > most) most = s.n;
    if (s.n == 0) continue;
    if (s.y != rr % ey || s.z != rr / ey) ++bad;
    uint32_t g = (s.z * ey + s.y) * ex + s.x, y = s.y, y2 = s.y;
    int32_t l = (int32_t)g, l2 = 0;
    uint64_t t = 0;
    for (uint32_t k = 0; k < s.n; ++k) {
      const uint32_t row = rr + k * per;  // the row this lane moves in pass k
      if (row >= rows || g != row * ex + s.x || (uint32_t)l != g || y != row % ey) {
        ++bad;
        break;
      }
      if ((uint32_t)t != k * per || (uint32_t)(t >> 32) != row / ey - s.z) ++bad;
      for (int e = 0; e < V; ++e) {
        if (g + e >= vol) {  // (kept from the buffers in the plain build: counted, not performed)
          ++bad;
          continue;
        }
        slot[l + e] = src[g + e];
        ++writes[l + e];
        ++moved;
      }
      vr::stage_next(M, S, g, l, y);
      vr::stage_next(M, T, t, l2, y2);
    }
    if (rr + s.n * per < rows) ++bad;  // no row of the lane's is left
  }
  if (most != passes) ++bad;
  for (uint32_t i = 0; i < vol; ++i)
    if (writes[i] == 0 || slot[i] != src[i]) ++bad;
  delete[] src;
  delete[] slot;
  ++boxes;
}

int main() {
  for (uint32_t ex = 1; ex <= 64; ++ex)
    for (uint32_t ey = 1; ex * ey <= 2560; ++ey)
      for (uint32_t ez = 1; ex * ey * ez <= 2560; ++ez) {
        run_box<1>(ex, ey, ez);
        if (ex >= 2) run_box<2>(ex, ey, ez);
        if (ex >= 4) run_box<4>(ex, ey, ez);
        // a row narrower than the width takes the next narrower one
        const int w4 = vr::stage_width(ex, 4), w2 = vr::stage_width(ex, 2), w1 = vr::stage_width(ex, 1);
        if (w4 != (ex >= 4 ? 4 : ex >= 2 ? 2 : 1) || w2 != (ex >= 2 ? 2 : 1) || w1 != 1) ++bad;
      }
  printf("boxes %ld moved %ld mismatches %ld\n", boxes, moved, bad);
  return 0;
}
"""


def compiler():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def build_and_run(tmp_path, name, flags):
    cxx = compiler()
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    cc = subprocess.run([cxx, "-std=c++17", "-O2", "-I", CSRC] + flags + [str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=300)
    assert not out.stderr.strip(), out.stderr
    return out.stdout.split()


def check(words):
    # every box, at each width its rows can take
    want = sum((ex >= 1) + (ex >= 2) + (ex >= 4) for ex in range(1, 65) for ey in range(1, 2560 // ex + 1)
               for ez in range(1, 2560 // (ex * ey) + 1))
    assert words[0] == "boxes" and int(words[1]) == want, (words, want)
    assert words[2] == "moved" and int(words[3]) > 0, words
    assert words[4] == "mismatches" and int(words[5]) == 0, words


def test_stage_map_moves_every_box(tmp_path):
    """Every box element is written, every write carries its source element, nothing outside the box
    is touched, no lane reads outside [0, ex) of its row, and the pass count is ceil(rows / (64 / gx));
    0 mismatches."""
    check(build_and_run(tmp_path, "stage_map_check", []))


def test_stage_map_under_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run directly: no report, 0 mismatches."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # whether the compiler has the sanitizers' runtimes at all: an empty program, before any work (a
    # failure of the real program below fails the test)
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    cc = subprocess.run([compiler(), "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")],
                        capture_output=True, text=True)
    if cc.returncode:
        pytest.skip("the host compiler cannot link -fsanitize=address,undefined (the plain build is tested above)")
    check(build_and_run(tmp_path, "stage_map_check_san", flags))
