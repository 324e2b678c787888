"""The arithmetic of the BP host staging (csrc/host_pipe_plan.hpp) without a GPU: the staging image layout, the chunk rule
of the large-batch pipeline, and span_of + merge_bit_range of the bit-packed entry, driven by a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_pipe_plan_under_sanitizers(tmp_path):
    """csrc/host_pipe_plan.hpp built with a plain C++ compiler (it includes no HIP) under AddressSanitizer + UBSan, CPU
    only, and driven by tests/native/host_pipe_plan_sanitize.cpp: the chunk rule against hand-derived values, the layout
    against the hand-written carving, merge_bit_range against a bit-by-bit model for every offset 0..63 and length 0..200
    with buffers of exactly the covering word count."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "host_pipe_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *san, "-I", os.path.join(ROOT, "ldpcdecoders.jl_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "host_pipe_plan_sanitize.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK host pipe plan") and "25728 merges" in out.stdout, out.stdout + out.stderr
