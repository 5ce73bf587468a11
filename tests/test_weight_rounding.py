"""The 8-bit filter weights without v_rndne (vr_sampling.h weight8_rn / frac8_rn) against the rintf
forms on the CPU: tools/microbench/weight8_check.c over every 97th fp32 of both ranges plus every
tie k / 512 (the full ranges run with stride 1, by hand)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_weight_forms_agree_bit_for_bit(tmp_path):
    exe = str(tmp_path / "weight8_check")
    src = os.path.join(ROOT, "tools", "microbench", "weight8_check.c")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True)
    p = subprocess.run([exe, "97"], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    fields = dict(kv.split("=") for kv in p.stdout.split())
    assert int(fields["bad"]) == 0
    assert int(fields["n"]) > 30_000_000  # both ranges and the ties were visited
