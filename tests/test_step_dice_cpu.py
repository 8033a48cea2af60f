"""LaneRng::step_dice (ewn_gym_amd/csrc/ewn_core.hpp): the two dice of an env step taken at once from the step's primed Philox block
must be what two randint(1, 7) on the same stream return, stream positions included -- on the straight path (both low halves of
the Lemire products at or above 6) and through the one cold block (a rejected first draw shifts the second; a rejection in a
block's last word goes on into the next block).

All on the host: tests/step_dice_host.hip calls the function itself (compiled here for the host alone, a second or two)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tallies(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_dice") / "step_dice_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ewn_gym_amd", "csrc"),
                           os.path.join(ROOT, "tests", "step_dice_host.hip"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-2000:]
    out = {}
    for line in p.stdout.splitlines():
        f = line.split()
        out[f[0]] = dict(zip(f[1::2], (int(x) for x in f[2::2])))
    return out


def test_seeded_and_random_blocks_take_the_straight_path(tallies):
    for group in ("philox", "random"):
        t = tallies[group]
        assert t["cases"] == 4096 and t["cold"] == 0 and t["shifted"] == 0 and t["crossed"] == 0, (group, t)


def test_each_edge_word_in_either_place_takes_the_cold_block(tallies):
    # of the six words w with (u32)(w * 6) < 6 four are rejected (low half below 2^32 mod 6 = 4): k = 0, 1, 3, 4
    assert tallies["edge_b0"] == {"cases": 48, "cold": 48, "shifted": 32, "crossed": 0}
    assert tallies["edge_b1"] == {"cases": 48, "cold": 48, "shifted": 32, "crossed": 0}
    t = tallies["edge_b0_b1"]
    assert t["cases"] == 288 and t["cold"] == 288 and t["shifted"] == 288 - 8 * 4 and t["crossed"] == 0, t


def test_rejections_through_the_last_word_cross_into_the_next_block(tallies):
    t = tallies["last_word"]
    # no ordinary word, or only the first: the draws run off the block's end; two or three ordinary words in front: the straight path
    assert t == {"cases": 64, "cold": 32, "shifted": 32, "crossed": 32}, t
