"""Builds and runs a stand-alone host program of tools/ (plain C++ over a header of gim_amd/csrc), for the CPU tests that compare
its output with the numpy restatement of the same kernel."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(name, out_dir, *flags):
    """tools/<name>.cpp compiled as C++17 at -O1 (plus `flags`, e.g. "-ffp-contract=off") with the host compiler and -I gim_amd/csrc,
    then run; both steps must exit with 0 -> the run's CompletedProcess (stdout, stderr as text)"""
    from gim_amd.build import _hipcc
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or _hipcc()   # hipcc compiles plain C++ too
    exe = os.path.join(str(out_dir), name)
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "gim_amd", "csrc"),
                        os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r
