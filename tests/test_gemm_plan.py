"""CPU: how a projection runs, pinned.  plan_gemm() (gist_amd/csrc/gemm_plan.cpp) decides path, tile, k slices, tail
units, scratch and launch count for every launcher and every size query of the GEMM family; gist_gemm_plan_query returns
its record without touching a device.  This file asks it about every projection of the benchmark configurations, at the
batch sizes around the tile and round boundaries, in each GEMM mode, for each kind of call, under each tuning hook and
with too little scratch, and compares the records with recorded ones.

The expected records (tests/golden/gemm_plan_parent.json) were NOT produced by the code under test.  The whole table is
several hundred thousand plans, too many to keep as text: the file holds, one per line, the plans of a subset that reaches every branch
(one case per distinct combination of path, tile, slice count, tail form and what one byte less of scratch does to them,
per kind of call and per hook, plus the shapes named below), and one SHA-256 per (mode, hooks) group over ALL of that
group's cases, scratch values and records.  A digest that differs says that some plan of the group differs; the pinned
subset usually says which.  Both come from the decision functions of commit 5d254ba, the last one in which the launchers and the size queries each computed them on their own: a build of that
commit with a scratch-only patch that exported its choose_cfg, h3_shape_ok, b3_shape_ok, b3_splits, b3_tail, b3_wide,
b3c_shape_ok, b3c_choice, b3c_tail and the byte formulas untouched, combined the way that commit's launchers combined
them, run over cases() below.  The old size queries (sections "queries", the answers without hooks, and "query_digests")
were recorded from that build's C ABI directly.

To regenerate (after a change that is MEANT to alter a decision, from the commit before it): export the functions above
through extern "C" wrappers that only forward their arguments; for every group of GROUPS set mode and hooks, and for every
case of cases() compose the record as that commit's launch_gemm / h3_gemm / b3_gemm / b3_gemm_presplit / b3c_gemm did,
fields in FIELDS' order (scratch_bytes = slices asked for after the scratch rule x m x n x 4, or the tail partials in use;
k = 0: the fp32 kernel, whatever the kind of call).  A group's digest is digest() over the concatenation, case by case in
cases()' order and for each case scratch by scratch in scratches()' order (computed from the workspace_bytes of that
case's unbounded plan), of the 23 integers [layout, m, n, k, aligned, call, deferred, scratch, the 15 fields]; a query
digest is digest() over old_queries()' answers in its order.  digest() packs little-endian int64.

Everything is an integer and deterministic: the margin is zero."""
import ctypes
import hashlib
import itertools
import json
import os
import struct

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_plan_parent.json')
FIELDS = ('path', 'kept_ok', 'tile_m', 'tile_n', 'splits', 'whole_tiles', 'tail_splits', 'launches', 'k_per_split',
          'tail_k', 'operand_offset', 'operand_bytes', 'scratch_offset', 'scratch_bytes', 'workspace_bytes')
F32, H3, B3, B3C = 0, 1, 2, 3                      # GIST_GEMM_PATH_*
SPLITS, KEPT, SLABS = 0, 1, 2                      # GIST_GEMM_CALL_*
NT, NN, TN = 0, 1, 2

# (n_in, n_out) of every layer: bench config 3 at four widths, config 2, config 4 (one rank's 512-wide sub-model)
LAYERS = [d for H in (4096, 2048, 1024, 512) for d in ((602, H), (H, H), (H, 41))] + \
         [(100, 256), (256, 256), (256, 12)] + [(100, 512), (512, 47)]
ROWS = (500, 2046, 2049, 2100, 2150, 2304)
# shapes outside the layer table that reach a branch it does not: 32 fp32 slices, a skinny output of many k tiles, and an
# empty reduction (k = 0: bias or zeros from the fp32 kernel, in every mode and for every kind of call)
EXTRA = [(TN, 12, 512, 8192), (TN, 41, 64, 16384), (NT, 2100, 4096, 1024), (NT, 300, 200, 0), (NN, 300, 200, 0), (TN, 300, 200, 0)]


def shapes():
    """(layout, m, n, k) of Y = Z . W^T, dZ = dY . W and dW = dY^T . Z of every layer at every batch size."""
    out = []
    for (i, o), r in itertools.product(LAYERS, ROWS):
        out += [(NT, r, o, 2 * i), (NN, r, 2 * i, o), (TN, o, 2 * i, r)]
    return out + EXTRA


# tuning hooks (gist_amd/_lib.py TUNE), each set for its group of cases and cleared after it; and the modes it bears on
HOOKS = [
    ({}, (0, 1, 2)),
    ({'gemm_tile': 64, 'gemm_splits': 4}, (0, 1, 2)),
    ({'gemm_tile': 128, 'gemm_splits': 16}, (0, 2)),
    ({'gemm_tile': 128128, 'gemm_splits': 2}, (2,)),
    ({'h3_min_tiles': 1, 'h3_min_gflop': 0.001}, (1, 2)),
    ({'h3_min_gflop': 40.0}, (1, 2)),
    ({'h3_tm': 64}, (1,)),
    ({'h3_tm': 128}, (1,)),
    ({'b3c': 1}, (2,)),
    ({'b3c': 2}, (2,)),
    ({'b3c': 2, 'b3c_splits': 3}, (2,)),
    ({'b3c_splits': 2}, (2,)),
    ({'b3_tail': 1}, (2,)),
    ({'b3_wide': 1}, (2,)),
    ({'gemm_dual': 1}, (0, 2)),
]
GROUPS = [(mode, hi) for hi, (_, modes) in enumerate(HOOKS) for mode in modes]


def cases():
    """Every query of a (mode, hooks) group but its scratch: (layout, m, n, k, aligned, call, deferred)."""
    return [(lay, m, n, k, al, call, d)
            for (lay, m, n, k) in shapes() for al in (1, 0) for call in (SPLITS, KEPT, SLABS) for d in (0, 1)]


def scratches(need):
    """Scratch on hand, given what the plan with unbounded scratch asks for: unbounded, and (where it asks for any)
    nothing, one byte too little, exactly that."""
    return (-1, 0, need - 1, need) if need > 0 else (-1, 0)


def digest(ints):
    return hashlib.sha256(struct.pack('<%dq' % len(ints), *ints)).hexdigest()


class Hooks:
    """Set a group's mode and hooks; restore both."""

    def __init__(self, L, mode, hooks):
        self.L, self.mode, self.hooks = L, mode, hooks

    def __enter__(self):
        from gist_amd import _lib
        self.prev = self.L.gist_gemm_get_mode()
        assert self.L.gist_gemm_set_mode(self.mode) == 0
        for name, v in self.hooks.items():
            assert self.L.gist_tuning_get(_lib.TUNE[name]) == 0.0
            assert self.L.gist_tuning_set(_lib.TUNE[name], float(v)) == 0

    def __exit__(self, *exc):
        from gist_amd import _lib
        for name in self.hooks:
            self.L.gist_tuning_set(_lib.TUNE[name], 0.0)
        self.L.gist_gemm_set_mode(self.prev)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g['fields'] == list(FIELDS) and g['groups'] == [list(x) for x in GROUPS]
    # pinned row: [group, layout, m, n, k, aligned, call, deferred, scratch, the record's fields]
    g['pinned'] = [(r[0], tuple(r[1:8]), r[8], tuple(r[9:])) for r in g['pinned']]
    return g


@pytest.fixture(scope='module')
def lib():
    from gist_amd import _lib
    return _lib.load()


def query(L, out, lay, m, n, k, al, call, d, scratch):
    assert L.gist_gemm_plan_query(lay, m, n, k, al, call, d, scratch, ctypes.byref(out)) == 0
    return struct.unpack('8i7q', bytes(out))


GROUP_IDS = ['mode%d-%s' % (m, '+'.join('%s=%g' % kv for kv in HOOKS[h][0].items()) or 'plain') for m, h in GROUPS]


@pytest.mark.parametrize('gi', range(len(GROUPS)), ids=GROUP_IDS)
def test_pinned_plans_match_the_parent_commits_decisions(lib, golden, gi):
    from gist_amd import _lib
    mode, hi = GROUPS[gi]
    out = _lib.GemmPlan()
    rows = [r for r in golden['pinned'] if r[0] == gi]
    assert rows
    with Hooks(lib, mode, HOOKS[hi][0]):
        bad = [(c, s, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))
               for (_, c, s, want) in rows for got in [query(lib, out, *c, s)] if got != want]
    assert not bad, '%d plans differ, the first (case, scratch, got, parent): %r' % (len(bad), bad[0])
    for name in HOOKS[hi][0]:
        assert lib.gist_tuning_get(_lib.TUNE[name]) == 0.0


@pytest.mark.parametrize('gi', range(len(GROUPS)), ids=GROUP_IDS)
def test_every_plan_of_the_table_matches_the_parent_commits_decisions(lib, golden, gi):
    from gist_amd import _lib
    mode, hi = GROUPS[gi]
    out = _lib.GemmPlan()
    stream = []
    with Hooks(lib, mode, HOOKS[hi][0]):
        for c in cases():
            full = query(lib, out, *c, -1)
            for s in scratches(full[FIELDS.index('workspace_bytes')]):
                r = full if s == -1 else query(lib, out, *c, s)
                assert s != full[-1] or r == full, (c, s, r, full)      # exactly what it asks: the same plan
                stream += list(c) + [s] + list(r)
    assert digest(stream) == golden['digests'][gi], 'a plan among the %d of this group differs from the parent commit' % (len(stream) // 23)


def test_the_pinned_plans_reach_every_branch(golden):
    """Over the recorded plans alone: every path, tile, slice count, tail form and scratch rule occurs."""
    rows = [(GROUPS[gi], c, s, dict(zip(FIELDS, r))) for (gi, c, s, r) in golden['pinned']]
    plain = [(c, s, r) for ((mode, hi), c, s, r) in rows if not HOOKS[hi][0]]
    every = [(c, s, r) for (_, c, s, r) in rows]

    def some(pool, **want):
        return any(all(r[k] == v if not callable(v) else v(r[k]) for k, v in want.items()) for (_, _, r) in pool)

    assert {r['path'] for (_, _, r) in plain} == {F32, H3, B3, B3C}
    # an empty reduction: the fp32 kernel writes bias or zeros, in every mode and for every kind of call
    empty = [((mode, c[0], c[5]), r) for ((mode, hi), c, s, r) in rows if c[3] == 0]
    assert {key for key, _ in empty} == set(itertools.product((0, 1, 2), (NT, NN, TN), (SPLITS, KEPT, SLABS)))
    for _, r in empty:
        assert (r['path'], r['splits'], r['k_per_split'], r['launches'], r['workspace_bytes'], r['kept_ok']) == (F32, 1, 64, 1, 0, 0)
    # bf16x3 on pre-split operands: one slice, 2-4 slices, tail units, the 256 x 256 tile; kept and per call
    for call in (SPLITS, KEPT):
        pool = [(c, s, r) for (c, s, r) in plain if c[5] == call and s == -1 and r['path'] == B3]
        assert some(pool, splits=1, tail_splits=1, tile_n=128)
        assert some(pool, splits=lambda v: 2 <= v <= 4)
        assert some(pool, tail_splits=lambda v: v > 1, tile_n=128)
        assert some(pool, tile_n=256, splits=1, tail_splits=1)
    named = {(c[1], c[2], c[3]): r for (c, s, r) in plain if s == -1 and c[5] == KEPT and r['path'] == B3}
    assert 2 <= named[(4096, 1204, 2046)]['splits'] <= 4                    # an output of 129-191 tiles
    assert named[(2100, 4096, 8192)]['tail_splits'] > 1
    assert named[(4096, 8192, 2046)]['tile_n'] == 256 and named[(2046, 8192, 4096)]['tile_n'] == 256
    # convert on load: its three tiles (128 x 64 only through the tile hook), tail units at 64 x 64 and at 128 x 128
    c3 = [(c, s, r) for (c, s, r) in every if r['path'] == B3C]
    assert {(r['tile_m'], r['tile_n']) for (_, _, r) in c3} == {(64, 64), (128, 64), (128, 128)}
    c3_plain = {(c[1], c[2], c[3]): r for (c, s, r) in plain if s == -1 and r['path'] == B3C}
    assert c3_plain[(2100, 1024, 2048)]['tail_splits'] > 1 and c3_plain[(2100, 1024, 2048)]['tile_m'] == 64
    assert some([x for x in c3 if x[1] == -1], tile_m=128, tile_n=128, tail_splits=lambda v: v > 1)
    assert some(c3, splits=lambda v: v > 1)
    # fp32: both tiles, every slice count of the model
    f32 = [(c, s, r) for (c, s, r) in plain if r['path'] == F32 and s == -1]
    assert {r['tile_m'] for (_, _, r) in f32} == {64, 128}
    assert {1, 2, 4, 8, 16, 32} <= {r['splits'] for (_, _, r) in f32}
    # f16x3: both A-tile heights, both kinds of pre-pass
    h3 = [(c, s, r) for (c, s, r) in plain if r['path'] == H3]
    assert {r['tile_m'] for (_, _, r) in h3} == {64, 128}
    assert {r['launches'] for (c, _, r) in h3 if c[5] == SPLITS} == {3, 4, 5}
    # the scratch rules: one byte too little and ...
    by_case = {}
    for (c, s, r) in plain:
        by_case.setdefault(c, {})[s] = r
    halved = one_b3 = one_c3 = whole_b3 = whole_c3 = next_path = 0
    for c, v in by_case.items():
        full = v[-1]
        need = full['workspace_bytes']
        if need <= 0:
            continue
        less = v[need - 1]
        assert v.get(need, full) == full and (0 not in v or v[0]['workspace_bytes'] == 0), (c, v)
        same = less['path'] == full['path']
        halved += same and full['path'] == F32 and 1 < less['splits'] < full['splits']       # ... the fp32 path halves
        one_b3 += same and full['path'] == B3 and full['splits'] > 1 and less['splits'] == 1  # ... bf16x3 runs one slice
        one_c3 += same and full['path'] == B3C and full['splits'] > 1 and less['splits'] == 1
        whole_b3 += same and full['path'] == B3 and full['tail_splits'] > 1 and less['tail_splits'] == 1   # ... whole tiles
        whole_c3 += same and full['path'] == B3C and full['tail_splits'] > 1 and less['tail_splits'] == 1
        next_path += full['operand_bytes'] > 0 and less['operand_bytes'] == 0   # ... a call cannot split its operands
    assert halved and one_b3 and whole_b3 and whole_c3 and next_path, (halved, one_b3, one_c3, whole_b3, whole_c3, next_path)
    # (k slices on the convert-on-load path exist only under a hook: its rule is met there)
    hooked = {}
    for ((mode, hi), c, s, r) in rows:
        hooked.setdefault((mode, hi, c), {})[s] = r
    assert any(v[-1]['path'] == B3C and v[-1]['splits'] > 1 and v[-1]['workspace_bytes'] - 1 in v and
               v[v[-1]['workspace_bytes'] - 1]['path'] == B3C and v[v[-1]['workspace_bytes'] - 1]['splits'] == 1
               for v in hooked.values())


# ---- the size queries that existed before the plan: the same values as before -----------------------------------
def step_plan(dims, n_max):
    from gist_amd import _lib
    P = _lib.StepPlan()
    P.n_layers, P.use_layernorm, P.p_drop = len(dims), 1, 0.2
    for k, (i, o) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out = i, o
        P.layer[k].ldz, P.layer[k].ldy = 2 * i, o if o % 4 == 0 else (o + 3) // 4 * 4
    P.n_max, P.feat_absmax = n_max, 5.0
    return P


def gat_plan(dims, n_max):
    from gist_amd import _lib
    P = _lib.GATStepPlan()
    P.n_layers, P.n_max = len(dims), n_max
    for k, (i, o, h) in enumerate(dims):
        P.layer[k].n_in, P.layer[k].n_out, P.layer[k].heads = i, o, h
    return P


STEP_PLANS = [([(602, H), (H, H), (H, 41)], n) for H in (4096, 2048, 1024, 512) for n in (2046, 2200, 2304)] + \
             [([(100, 256), (256, 256), (256, 256), (256, 12)], 2046), ([(100, 512), (512, 512), (512, 512), (512, 512), (512, 47)], 1200)]
# (the plans of tests/test_gat_step_exports.py; the SAGE plan of tests/test_cabi_exports.py is STEP_PLANS[1])
GAT_PLANS = [([(50, 32, 4), (32, 5, 1)], 300), ([(602, 64, 4), (64, 64, 4), (64, 41, 1)], 2200),
             ([(7, 30, 1), (30, 30, 1), (30, 3, 1)], 97)]


# Two hook settings under which the step's slab sizes are MEANT to differ from the parent commit's: its sizing took flags
# (tail, tn) in place of the layout -- a TN weight gradient got no tail partials even where GIST_TUNE_B3C = 2 sends it to the
# convert-on-load kernel, and got that kernel's forced slices (GIST_TUNE_B3C_SPLITS) even where it stays on the fp32 kernel.
# The plan sizes what the launcher will run.  Their fused-step sizes are left out; everything else is pinned there too.
FUSED_SIZES_FOLLOW_THE_LAYOUT = [{'b3c': 2}, {'b3c_splits': 2}]


def old_queries(L, fused=True):
    """[(name, args, value)] of every size query that predates the plan, under the current mode and hooks."""
    out = []
    for (lay, m, n, k) in shapes():
        if lay == NT:      # (the two queries take no layout: once per shape)
            out.append(('gist_gemm_workspace_bytes', [m, n, k], L.gist_gemm_workspace_bytes(m, n, k)))
            out.append(('gist_gemm_splits_operands', [m, n, k], L.gist_gemm_splits_operands(m, n, k)))
    for (i, o), r in itertools.product(LAYERS, ROWS):
        lddy = (o + 3) // 4 * 4
        out.append(('gist_gemm_dual_takes', [r, 2 * i, o],
                    L.gist_gemm_dual_takes(r, 2 * i, o, lddy, 2 * i, 2 * i, 2 * i, 4096, 4096, 4096, 4096)))
    for pi, (dims, n_max) in enumerate(STEP_PLANS):
        P = step_plan(dims, n_max)
        for mode in (0, 1, 2):
            out.append(('gist_step_h3_workspace_bytes_mode', [pi, mode], L.gist_step_h3_workspace_bytes_mode(ctypes.byref(P), mode)))
        if fused:
            out.append(('gist_step_fused_workspace_bytes', [pi], L.gist_step_fused_workspace_bytes(ctypes.byref(P))))
        for k in range(len(dims) + 2 if fused else 0):
            out.append(('gist_step_fused_slab_bytes', [pi, k], L.gist_step_fused_slab_bytes(ctypes.byref(P), k)))
        out.append(('gist_step_col_partials_floats', [pi], L.gist_step_col_partials_floats(ctypes.byref(P))))
    for pi, (dims, n_max) in enumerate(GAT_PLANS):
        P = gat_plan(dims, n_max)
        out.append(('gist_gat_step_workspace_bytes', [pi], L.gist_gat_step_workspace_bytes(ctypes.byref(P))))
    return out


@pytest.mark.parametrize('gi', range(len(GROUPS)), ids=GROUP_IDS)
def test_old_size_queries_answer_as_the_parent_commit_did(lib, golden, gi):
    mode, hi = GROUPS[gi]
    with Hooks(lib, mode, HOOKS[hi][0]):
        got = old_queries(lib, HOOKS[hi][0] not in FUSED_SIZES_FOLLOW_THE_LAYOUT)
    assert got
    if str(gi) in golden['queries']:      # without hooks: every answer, in old_queries' order
        want = golden['queries'][str(gi)]
        assert len(got) == len(want)
        bad = [(g, w) for g, w in zip(got, want) if g[2] != w]
        assert not bad, '%d answers differ, the first ((query, arguments, answer), answer of the parent commit): %r' % (len(bad), bad[0])
    assert digest([int(v) for (_, _, v) in got]) == golden['query_digests'][gi]
