"""k-slam_amd/host/pileup_walk.hpp, what the host twins of the pile-up reports share (the fit check, the skip preamble, the
contributing set, the oriented query), alone: tests/pileup_walk.cpp walks its rules at their edges.  No GPU, no library."""
import os
import shutil
import subprocess


def test_pileup_walk_at_every_edge_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into Python) built with the address and undefined-behaviour
    sanitizers: every array is a heap block of exactly its size, so a rule that reads past one fails the run."""
    gxx = shutil.which("g++")
    assert gxx
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "pileup_walk.cpp")
    exe = str(tmp_path / "pileup_walk")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
