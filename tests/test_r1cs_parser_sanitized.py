"""The .r1cs reader of the product under AddressSanitizer + UBSan on the CPU: the trapdoor circuit's .r1cs, mutated a few
thousand times with a fixed seed -- bit flips, truncations, counts and sizes near 2^31, 2^32, 2^63 and 2^64 --, must end in a
normal return or a C++ exception every time, never in an out-of-bounds access (tests/native/fuzz_r1cs.cpp: a stand-alone
program of host code only, run directly)."""
import os
import subprocess

import pytest

import r1cs_cases as K
import sanitized_build


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("fuzz"), "fuzz_r1cs", ["fuzz_r1cs.cpp", "host_util.cpp"], need_gxx=False)


def test_mutated_r1cs_never_crashes_the_reader(harness, tmp_path):
    path = tmp_path / "trapdoor.r1cs"
    path.write_bytes(K.trapdoor()[2])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, str(path), "4000", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("0 crashed")
    parsed, rejected = int(r.stdout.split()[0]), int(r.stdout.split()[2])
    assert rejected > 1000 and parsed > 100 and parsed + rejected == 4000      # the mutations bite, some still parse, all accounted for
