"""The multiply-and-shift quotient of the staging copy (volume_renderer_amd/csrc/vr_udiv.h udiv_small,
urem_small and the table make_udiv_tab) against `/` and `%`, exhaustively over the helper's stated
bounds, in a stand-alone host program built with g++ (once plain, once with the address and
undefined-behaviour sanitizers, run directly)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volume_renderer_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "vr_udiv.h"

int main() {
  static_assert(vr::UDIV_MAX_N >= 2048 && vr::UDIV_MAX_D >= 64, "the bounds the staging copy relies on");
  const vr::UdivTab tab = vr::make_udiv_tab();
  long bad = 0, checked = 0;
  for (uint32_t d = 1; d <= vr::UDIV_MAX_D; ++d) {
    const uint32_t magic = vr::udiv_magic(d);
    if (tab.e[d].m != magic || tab.e[d].mper != vr::udiv_magic(64u / d)) ++bad;
    // the product must fit 32 bits and both factors 24 (the device multiplies 24-bit operands)
    if ((uint64_t)(vr::UDIV_MAX_N - 1) * magic > 0xffffffffull || magic >= (1u << 24)) ++bad;
    for (uint32_t n = 0; n < vr::UDIV_MAX_N; ++n) {
      const uint32_t q = vr::udiv_small(n, magic), r = vr::urem_small(n, q, d);
      if (q != n / d || r != n % d) ++bad;
      ++checked;
    }
  }
  // the staging copy's rows per pass, 64 / ex from the magic of ex, and the quotient by an extent
  // above 64 taken with the magic of 64 (dividends below 64: 0 either way)
  for (uint32_t d = 1; d <= 64; ++d)
    if (((64u * tab.e[d].m) >> vr::UDIV_SHIFT) != 64u / d) ++bad;
  for (uint32_t d = 65; d <= 4096; ++d)
    for (uint32_t n = 0; n < 64; ++n)
      if (vr::udiv_small(n, tab.e[64].m) != n / d || vr::urem_small(n, 0u, d) != n % d) ++bad;
  printf("checked %ld mismatches %ld\n", checked, bad);
  return 0;
}
"""


def build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC] + flags + [str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    if cc.returncode and flags and ("asan" in cc.stderr or "ubsan" in cc.stderr):
        pytest.skip("the host compiler has no sanitizer runtime (the plain build is tested above)")
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120)
    assert not out.stderr.strip(), out.stderr
    return out.stdout.split()


def test_udiv_small_matches_division(tmp_path):
    """Every n in [0, 4096) (the issue's [0, 2048) and the dividends up to the largest slot's row count
    plus 63) and every d in [1, 64]: quotient and remainder equal `/` and `%`; the table holds the
    magics; 0 mismatches."""
    words = build_and_run(tmp_path, "udiv_check", [])
    assert words[0] == "checked" and int(words[1]) >= 2048 * 64
    assert words[2] == "mismatches" and int(words[3]) == 0, words


def test_udiv_small_under_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined, run directly: no report, 0 mismatches."""
    words = build_and_run(tmp_path, "udiv_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert words[2] == "mismatches" and int(words[3]) == 0, words
