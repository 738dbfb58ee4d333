"""The lane -> LDS offset maps of the conv weight-grads' transposed operand reads (csrc/tr_maps.h), checked on the CPU: the
stand-alone program tools/host/tr_maps_check.cpp emulates ds_read_b64_tr_b16 on index-filled images and compares every
fragment element of all 64 lanes and every (step, tile) with the element-by-element gather the read replaces, and checks each
lane address for 8-byte alignment and bounds."""
import os
import shutil
import subprocess

import pytest


def _build_and_run(tmp_path, flags, tag):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    src = os.path.join(os.path.dirname(__file__), "..", "tools", "host", "tr_maps_check.cpp")
    exe = str(tmp_path / ("tr_maps_check" + tag))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, src, "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and flags and "sanitize" in (b.stderr or "").lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert b.returncode == 0, b.stderr[-2000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_transposed_read_maps_equal_the_gathers(tmp_path):
    r = _build_and_run(tmp_path, [], "")
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_transposed_read_maps_clean_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: an offset outside its image is a report."""
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"], "_san")
    assert r.returncode == 0 and "OK" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-3000:])
