"""The stream timer behind ug_ctx_timings and ug_ctx_kernel_stats (csrc/stream_timer.hpp): eager sections, the event pairs of a
recorded launch sequence, and abandoned work -- on the H-polynomial block of the 1 024-constraint fixture, one context, so a
recorded sequence has no parallel branches. Every count is exact: no sample is dropped, none is counted twice."""
import ctypes as C
import os

import pytest

import oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NTT = 2                # ug_ctx_kernel_stats: the NTT pass launches


@pytest.fixture(scope="module")
def block():
    zkey = open(os.path.join(GOLDEN, "circuit_final.zkey"), "rb").read()
    wtns = open(os.path.join(GOLDEN, "witness.wtns"), "rb").read()
    info = O.zkey_info(zkey)
    off, sz = O.section(zkey, "zkey", 4)
    coefs = zkey[off + 4:off + sz]
    off, sz = O.section(wtns, "wtns", 2)
    w = wtns[off:off + sz]
    h = O.hpoly(coefs, info["nCoefs"], w, info["nVars"], info["domainSize"])
    return dict(info=info, coefs=coefs, w=w, h=h)


def _setup(dev, block):
    info = block["info"]
    hp = dev.hpoly(block["coefs"], info["nCoefs"], info["domainSize"], info["nVars"])
    return hp, dev.dvec(info["nVars"], block["w"]), dev.dvec(info["domainSize"])


def _per_run(dev, hp, wv):
    """NTT pass launches of one block (switches the statistics on, leaves them at zero)"""
    dev.kernel_stats(which=NTT, reset=True)
    hp.run(wv)
    per_run = dev.kernel_stats(which=NTT, reset=True)[1]
    assert per_run > 0
    return per_run


def test_eager_accounting(device, block):
    import ultragroth_amd as ug
    dev = ug.Device(0)
    try:
        n = block["info"]["domainSize"]
        hp, wv, _ = _setup(dev, block)
        assert dev.download(hp.run(wv), 0, n) == block["h"]
        assert dev.kernel_stats(which=NTT)[1:] == (0, 0)                   # off until the first reset
        per_run = _per_run(dev, hp, wv)
        dev.timings(reset=True)
        k = 3
        for _ in range(k):
            hp.run(wv)
        _, launches, points = dev.kernel_stats(which=NTT)
        assert (launches, points) == (k * per_run, k * per_run * n)
        msm, fft = dev.timings(reset=True)
        assert fft > 0 and msm == 0
        assert dev.timings() == (0.0, 0.0)
    finally:
        dev.close()


def test_recorded_sequence_accounts_every_launch(device, block):
    L, h, n = device._L, device._h, block["info"]["domainSize"]
    hp, wv, out = _setup(device, block)
    assert L.ug_hpoly_run(hp.h, wv.h, out.h) == 0                          # eager once: the workspaces exist before the capture
    per_run = _per_run(device, hp, wv)
    device.timings(reset=True)
    graph = C.c_void_p()
    assert L.ug_graph_begin(h, None) == 0
    try:
        assert L.ug_hpoly_run(hp.h, wv.h, out.h) == 0
    finally:
        rc = L.ug_graph_end(h, C.byref(graph))
    assert rc == 0, L.ug_last_error()
    try:
        assert L.ug_graph_valid(graph) == 1
        assert L.ug_graph_launch(graph) == 0
        assert L.ug_graph_launch(graph) == 0                               # the first launch is accounted before its pairs are re-recorded
        assert L.ug_graph_launch(graph) == 0
        _, launches, points = device.kernel_stats(which=NTT)
        assert (launches, points) == (3 * per_run, 3 * per_run * n)
        msm, fft = device.timings()
        assert fft > 0 and msm == 0
        assert device.download(out, 0, n) == block["h"]
    finally:
        L.ug_graph_destroy(graph)


def test_abandoned_work_is_not_reported(device, block):
    L, h, n = device._L, device._h, block["info"]["domainSize"]
    hp, wv, out = _setup(device, block)
    per_run = _per_run(device, hp, wv)
    device.timings(reset=True)
    assert L.ug_hpoly_run(hp.h, wv.h, out.h) == 0
    L.ug_ctx_abandon(h)
    assert L.ug_hpoly_run(hp.h, wv.h, out.h) == 0
    assert L.ug_ctx_collect(h) == 0
    _, launches, points = device.kernel_stats(which=NTT)
    assert (launches, points) == (per_run, per_run * n)
    msm, fft = device.timings()
    assert fft > 0 and msm == 0
    assert device.download(out, 0, n) == block["h"]
