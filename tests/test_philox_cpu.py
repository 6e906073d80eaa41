"""The generator of the closed-loop noise on the host (ilqr_planner_amd/csrc/ilqr_noise.hpp, tests/cpp/philox_main.cpp): the published
known-answer vectors of Philox4x32-10, the map from a counter to two normals against the NumPy restatement of tests/closed_loop_noise.py, and
the per-step draw -- built plain, and as the same stand-alone program with -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from tests import closed_loop_noise as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = [(0, 0, 0, 0, 0), (12345, 3, 5, 7, 2), (0xDEADBEEFCAFEF00D, 4095, 63, 0xFFFFFFFF, 7), (1 << 63, 0xFFFFFFFF, 0xFFFFFFFF, 198, 0),
            (42, 12, 16, 8, 3)] + [(7, b, s, k, j) for b in (0, 12) for s in (0, 64) for k in (0, 398, 0xFFFFFFFF) for j in (0, 6)]


def test_restatement_reproduces_the_known_answers():
    for c, k, out in cn.KAT:
        assert tuple(int(v) for v in cn.philox4x32_10(*c, *k)) == out


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_generator_on_the_host(tmp_path, flags):
    exe, vec = str(tmp_path / "philox"), str(tmp_path / "normals.txt")
    with open(vec, "w") as f:
        for seed, b, s, k, j in COUNTERS:
            z0, z1 = cn.normals(seed, b, s, k, j)
            f.write(f"{seed} {b} {s} {k} {j} {float(z0).hex()} {float(z1).hex()}\n")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "philox_main.cpp"), "-o", exe])
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
    print(r.stdout.strip().splitlines()[-2])


def test_restatement_stream_is_sound():
    print(cn.check_stream(cn.draw(cn.SEED, 13, 17, range(8), 7), "restatement"))
    assert np.array_equal(cn.draw(cn.SEED, 13, 17, range(8), 7)[2:11, 1:14], cn.draw(cn.SEED, 9, 13, range(8), 7, 2, 1))
