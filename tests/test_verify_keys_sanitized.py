"""The host code of the calls under several keys under AddressSanitizer + UBSan on the CPU: verifier_api.cpp's keyed BatchCall with
device = -1 -- ragged inputs, the regrouping by key, the host forest, the search over the keys, the judge -- called by a stand-alone
program over random records (tests/native/verify_keys_main.cpp, built as tests/test_formats_sanitized.py builds its harness). Key
indices and input counts are a service's untrusted values: a call ends in verdicts or in a clean VERIFIER_ERROR."""
import os
import subprocess

import pytest

from conftest import GOLDEN
import sanitized_build


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("keys"), "verify_keys_main",
                                 ["verify_keys_main.cpp", "verifier_api.cpp", "verifier_records.cpp", "host_util.cpp"],
                                 flags=("-O1", "-pthread", "-Wno-unknown-pragmas"), need_gxx=False)


def test_keyed_calls_run_clean(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    td = os.path.join(GOLDEN, "trapdoor")
    args = ["5", "40", os.path.join(td, "ultra_vkey.json"), "1", os.path.join(td, "groth16_vkey.json"), "2",
            os.path.join(GOLDEN, "verification_key.json"), "1"]
    r = subprocess.run([harness] + args, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    calls, refused, verdicts, batched = int(words[0]), int(words[2]), int(words[4]), int(words[6])
    assert refused == 12 + 12 + 3 and calls == 18 + refused + 1 + 2 and verdicts == 18 * 40
    assert batched >= 3                                                         # compressed records did enter batches, and their search
