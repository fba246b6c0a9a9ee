"""The fixture body of the tests that run host code as a stand-alone program under AddressSanitizer + UBSan: probe for a
sanitizer runtime (only its absence may skip), compile, assert. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ultragroth_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(tmp, name, sources, flags=("-O1",), need_gxx=True):
    """g++ -std=c++17 <flags> -g <sanitizers> -I csrc -I include <sources> -o tmp/name; returns the program's path.
    sources: paths, or names looked up under tests/native and then under csrc. need_gxx = False: a machine without g++ skips."""
    if need_gxx:
        assert shutil.which("g++"), "no g++: the library's own Makefile needs one"
    elif not shutil.which("g++"):
        pytest.skip("no g++")
    probe = tmp / "probe.cpp"                      # is there a sanitizer runtime at all? only that may skip
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", SANITIZE[0], str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    paths = [s if os.path.isabs(s) else os.path.join(NATIVE if os.path.exists(os.path.join(NATIVE, s)) else CSRC, s) for s in sources]
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17"] + list(flags) + ["-g"] + SANITIZE + ["-I", CSRC, "-I", os.path.join(ROOT, "include")] + paths + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
