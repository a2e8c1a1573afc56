"""GPU: the windows and launch counters of scripts/measure.py on one small library call (hip.colsum on 64 x 64) and one
ATen kernel: the counts they return against the library's counter read directly around one call, and against the formula
the tools used before they shared this module.  No assertion on the size of any time."""
import math

import pytest
import torch

from scripts import measure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def calls():
    """-> (the library call, its launches read directly from the counter around one call, the ATen call)"""
    from gist_amd import _lib, hip
    L = _lib.load()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(64, 64, device=dev, generator=gen)
    out = torch.empty(64, device=dev)
    partials = torch.empty(max(L.gist_colsum_partials(64) * 64, 1), device=dev)
    a, b, c = torch.randn(64, 64, device=dev, generator=gen), torch.ones(64, 64, device=dev), torch.empty(64, 64, device=dev)

    def lib_call():
        hip.colsum(g, out, partials)

    def aten_call():
        torch.add(a, b, out=c)

    lib_call()
    aten_call()
    torch.cuda.synchronize()
    before = L.gist_launch_count()
    lib_call()
    direct = L.gist_launch_count() - before
    torch.cuda.synchronize()
    assert direct >= 1
    assert torch.allclose(out, g.sum(0), rtol=1e-5, atol=1e-5)
    return lib_call, direct, aten_call


def former_torch_launches(fn, dev):
    """scripts/graphsage_step.py's torch_launches as it stood before scripts/measure.py"""
    from torch.profiler import ProfilerActivity, profile
    from gist_amd import _lib
    L = _lib.load()
    torch.cuda.synchronize(dev)
    before = L.gist_launch_count()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(dev)
    ours = L.gist_launch_count() - before
    kernels = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                  and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    return max(kernels - ours, 0)


def test_event_window_times_and_counts(calls):
    lib_call, direct, _ = calls
    ms, launches = measure.event_window(lib_call, 8, count=True)
    assert math.isfinite(ms) and ms > 0
    assert launches == direct
    ms = measure.event_window(lib_call, 8)
    assert isinstance(ms, float) and math.isfinite(ms) and ms > 0


def test_host_window_times(calls):
    lib_call, _, _ = calls
    for dev in (None, torch.device('cuda', 0)):
        ms = measure.host_window(lib_call, 8, dev)
        assert math.isfinite(ms) and ms > 0


def test_lib_launches_and_launches_during_agree_with_the_counter(calls):
    lib_call, direct, aten_call = calls
    assert measure.lib_launches(lib_call, 5) == direct
    assert measure.lib_launches(aten_call, 5) == 0
    assert measure.launches_during(lambda: (lib_call(), lib_call(), 'done')[2]) == ('done', 2 * direct)


def test_torch_launches_counts_what_the_library_does_not(calls):
    lib_call, direct, aten_call = calls
    dev = torch.device('cuda', 0)
    assert measure.torch_launches(aten_call, dev) == 1
    assert measure.torch_launches(aten_call, dev) == former_torch_launches(aten_call, dev)
    # the library call alone: its kernels in the trace less its own count (0 where every kernel passes the counter)
    assert measure.torch_launches(lib_call, dev) == former_torch_launches(lib_call, dev)
    both = lambda: (lib_call(), aten_call())
    assert measure.torch_launches(both, dev) == former_torch_launches(both, dev)
