"""The host code of the record layouts under AddressSanitizer + UBSan on the CPU: pairing.hpp's square roots and decompression and
verifier_api.cpp's conversions, hooks and device = -1 batch path, called by a stand-alone program over random records
(tests/native/record_formats_main.cpp, built as tests/test_parsers_sanitized.py builds its harness). Records are a service's
untrusted bytes: a conversion ends in one of its return codes, a batch call in verdicts."""
import os
import subprocess

import pytest

from conftest import GOLDEN
import sanitized_build


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sanitized_build.build(tmp_path_factory.mktemp("formats"), "record_formats_main",
                                 ["record_formats_main.cpp", "verifier_api.cpp", "verifier_records.cpp", "host_util.cpp"],
                                 flags=("-O1", "-pthread", "-Wno-unknown-pragmas"), need_gxx=False)


def test_record_layouts_run_clean(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    key = os.path.join(GOLDEN, "trapdoor", "groth16_vkey.json")
    r = subprocess.run([harness, key, "48", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    converted, refused, with_root, values, verdicts = int(words[0]), int(words[2]), int(words[4]), int(words[6]), int(words[-2])
    assert converted + refused == 96 and converted >= 1 and refused >= 48       # both outcomes are met (a point has a y for about half the x)
    assert 8 <= with_root < values == 56 and verdicts == 48
