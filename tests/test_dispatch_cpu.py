"""csrc/acm_dispatch.h, the one translation from run-time values to kernel template arguments, as plain host C++: the program
tests/c_abi/dispatch_check.cpp includes only that header and checks what every launcher relies on."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_pick_reaches_every_listed_constant_once_and_nothing_else(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "dispatch_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "acm_gnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "dispatch_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "dispatch_check: ok" in out.stdout, (out.stdout, out.stderr)
