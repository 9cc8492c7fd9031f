"""k-slam_amd/host/batch_check.hpp, the one check of a batch's arrays in front of the reports' device entries and host twins,
alone: tests/batch_check.cpp walks its rules at their edges, level by level and message by message.  No GPU, no library."""
import os
import shutil
import subprocess


def test_batch_check_at_every_edge_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into Python) built with the address and undefined-behaviour
    sanitizers: every array is a heap block of exactly its size, so a rule that reads past one fails the run."""
    gxx = shutil.which("g++")
    assert gxx
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "batch_check.cpp")
    exe = str(tmp_path / "batch_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
