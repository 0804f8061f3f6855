"""The beam table's paired image (RcTrackDev::beam_pairs: two rounds' (cos, sin) pairs side by side, one 16-byte load per lane and
round pair in the one-wave-per-car scan) is a pure re-arrangement of the per-round table.  rc_load_track exposes no read-back, so
the re-arrangement is a small host function of its own (racing_dreamer_amd/csrc/racecar_beam_pairs.h, called by the upload) and
a stand-alone C++ program (tests/beam_pairs_check.cpp) checks it word for word.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "racing_dreamer_amd", "csrc")


def test_paired_beam_image_is_a_rearrangement_of_the_per_round_table(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "beam_pairs_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(HERE, "beam_pairs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines == ["beam_pairs_check beams: 2176 words in, 2304 words out, 0 wrong",
                     "beam_pairs_check patterns: 2176 words in, 2304 words out, 0 wrong"], r.stdout


def test_the_upload_builds_the_image_with_that_function():
    """The function under test is the one the library runs: rc_load_track's host tables call rc_pair_beams, the scan's one-wave
    builds read `beam_pairs` with a 16-byte load and every other build keeps the per-round table."""
    with open(os.path.join(CSRC, "racecar_abi.hip")) as f:
        abi = f.read()
    assert '#include "racecar_beam_pairs.h"' in abi and "rc_pair_beams(ht.beams.data(), ht.beam_pairs.data());" in abi
    assert "t.beam_pairs = (const float *)m" in abi
    from racing_dreamer_amd import build
    assert "racecar_beam_pairs.h" in build.HEADERS          # (part of the build id: a change to it rebuilds the library)
