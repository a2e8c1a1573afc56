"""The timing and counting rules of the tools under scripts/, stated once.

Three rules decide whether a row of a report is believed, and every tool takes them from here:

  warm-up first        every path finishes its warm-up before the first timed window of any path (the tool's own loop:
                       what a warm-up call is differs from tool to tool);
  alternating windows  `alternate`: in each of `reps` rounds every path runs one window, in the dict's order, so a drift
                       of the machine hits every path alike;
  every window         `every_window_shorter` / `verdict`: a path is called faster only where EVERY one of its windows is
                       shorter than EVERY window of the other; anything else, a tie included, is an overlap.

A window is `iters` back-to-back calls closed by ONE device-wide synchronise, so a time per call is the larger of the
host's issue time and the device time per call.  `event_window` reads it from two device events, `host_window` from the
host clock between two synchronisations (the whole loop body, an iterator's host work included).  Both return ms per
call; a tool that reports microseconds multiplies where it prints.  Launches are the library's own counter (COUNTER),
which sees the launches that pass through the library and none of ATen's; `torch_launches` counts the rest.

Plain functions; torch and the library are imported by the functions that need them, so the rules themselves (verdict,
alternate, cycle, stats) load without either."""
import os
import statistics
import time

COUNTER = 'gist_launch_count'


def require_gpu(tool):
    """A measurement path that finds no GPU fails; it never falls back."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('%s measures on the GPU; there is none here' % tool)


def _launch_count():
    from gist_amd import _lib
    return _lib.load().gist_launch_count


def event_window(fn, iters, count=False):
    """ms per call of `iters` calls between two device events, closed by one device synchronise; with count=True
    -> (ms, library launches per call), the counter read before the first event and after the synchronise"""
    import torch
    launched = _launch_count() if count else None
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0 = launched() if count else 0
    a.record()
    for _ in range(iters):
        fn()
    z.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(z) / iters
    return (ms, (launched() - c0) / float(iters)) if count else ms


def host_window(fn, iters, dev=None):
    """ms per call of `iters` calls on the host clock, between two device synchronisations"""
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / iters


def launches_during(fn):
    """-> (what fn() returns, the library launches it issued)"""
    launched = _launch_count()
    before = launched()
    res = fn()
    return res, launched() - before


def lib_launches(fn, iters):
    """library launches per call over `iters` calls"""
    launched = _launch_count()
    before = launched()
    for _ in range(iters):
        fn()
    return (launched() - before) / float(iters)


def torch_launches(fn, dev):
    """device kernels of one call that the library's counter does not see: ATen's, and the few library kernels that
    do not pass through its counter"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    launched = _launch_count()
    torch.cuda.synchronize(dev)
    before = launched()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(dev)
    ours = launched() - before
    kernels = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                  and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    return max(kernels - ours, 0)


def alternate(paths, window, reps, before=None):
    """{name: [window(fn) per round]} for paths = {name: fn}: `reps` rounds, every path once per round in the dict's
    order; before(name), when given, runs immediately ahead of each window (to put a setting in force).  Warm-up is the
    caller's, and complete for every path before this is called."""
    out = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            if before is not None:
                before(name)
            out[name].append(window(fn))
    return out


def split_counts(wins):
    """alternate()'s result over windows of event_window(..., count=True) -> ({name: [ms]}, {name: [launches per call]})"""
    return tuple({name: [w[j] for w in ws] for name, ws in wins.items()} for j in (0, 1))


def every_window_shorter(a, b):
    """the only claim a row may make: every window of a is shorter than every window of b (strictly: a tie overlaps)"""
    return max(a) < min(b)


def verdict(a, b, a_name, b_name, style='faster'):
    """the every-window rule in the wording of the committed reports: style 'faster' -> '<name> faster' / 'within the
    spread', style 'windows' -> 'every <x> window is shorter than every <y> window' / 'the windows overlap'"""
    assert style in ('faster', 'windows'), style
    for x, y, x_name, y_name in ((a, b, a_name, b_name), (b, a, b_name, a_name)):
        if every_window_shorter(x, y):
            if style == 'faster':
                return x_name + ' faster'
            return 'every %s window is shorter than every %s window' % (x_name, y_name)
    return 'within the spread' if style == 'faster' else 'the windows overlap'


def summary(ws):
    """(median, min, max) of the windows"""
    return statistics.median(ws), min(ws), max(ws)


def cell(ws, digits=3):
    """'median (min .. max)' of the windows, as the reports' tables print it"""
    return ('%%.%df (%%.%df .. %%.%df)' % ((digits,) * 3)) % summary(ws)


def spread(v):
    """run-to-run spread of the windows: (max - min) / median"""
    return (max(v) - min(v)) / float(statistics.median(v))


def stats(ws):
    return dict(median=round(float(statistics.median(ws)), 4), min=round(min(ws), 4), max=round(max(ws), 4),
                windows=[round(w, 4) for w in ws])


def cycle(it):
    """the elements of `it`, pass after pass, without end (`it` is iterated anew for every pass)"""
    while True:
        for b in it:
            yield b


def reference_loop(model, it, loss_f, opt, dev):
    """The reference's loop body (cluster_gcn.py:96-105, as main_module_path runs it) on `model` and the batches that
    next(it) gives, as one closure that returns the loss; weight decay, if any, is in `opt`."""
    def one():
        cluster = next(it).to(dev)
        model.train()
        pred = model(cluster)
        labels, mask = cluster.ndata['label'], cluster.ndata['train_mask']
        loss = loss_f(pred[mask], labels[mask])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return one


def write_lines(path, lines):
    """the tail of the markdown tools: the lines into `path` (its folder made if need be) and onto the screen"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
