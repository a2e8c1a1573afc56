"""TEST INFRASTRUCTURE (not product) for the GIST-for-BaselineGCN tests: a numpy restatement of the split table of
gist_amd.ist.DistributedBaselineGCNWrapper -- the reference's GCN dispatch / sync (cluster_gcn_ist_distrib.py:197-367)
transposed for GraphConv's [in, out] weight and without the concatenated half -- and a check_round over it.  A model is
[(W [in, out], b [out])] per layer as float32 arrays: every move is a copy, so everything is compared bit for bit.

The shared last bias is the fp32 mean of the sites' copies in site order.  Two summation orders exist in the product and
both are restated: the per-tensor double of the CPU tests (tests/gat_ist_restatement.TorchBlocks.mean_rows) adds the
sites one after the other; the HIP movers (csrc/mean_tree.h, shared by gist_mean_rows_f32 and the grouped mover) add
them pairwise.  At S = 2 the two are the same sum.  TorchBlocks, ref_sample and perturb are tests/gat_ist_restatement.py's."""
import random

import numpy as np
import torch

from tests.gat_ist_restatement import TorchBlocks, perturb, ref_sample        # noqa: F401  (re-exported)


def _idx(part, site):
    """idx_k of `site` for every partition (create_partition's `full` is not used by this family)."""
    return [np.asarray(layer[site][0], dtype=np.int64) for layer in part]


def _blocks(n_layers, part, site):
    """Per layer (rows, cols) of the block of W that `site` owns, None = all; the bias takes cols."""
    idx = _idx(part, site)
    last = n_layers - 1
    return [(idx[k - 1] if k > 0 else None, idx[k] if k < last else None) for k in range(n_layers)]


def ref_dispatch(base, part, site):
    """The sub-model of `site` sliced from `base`."""
    sub = []
    for (W, b), (rows, cols) in zip(base, _blocks(len(base), part, site)):
        W = W if rows is None else W[rows, :]
        W = W if cols is None else W[:, cols]
        sub.append((np.ascontiguousarray(W), (b if cols is None else b[cols]).copy()))
    return sub


def site_mean(vectors, tree=False):
    """The fp32 mean of the sites' vectors in site order: one after the other from zero, or pairwise as
    csrc/mean_tree.h adds them (64 slots, zero beyond the sites)."""
    n = np.float32(len(vectors))
    if not tree:
        acc = np.zeros_like(vectors[0], dtype=np.float32)
        for v in vectors:
            acc = acc + v.astype(np.float32)
        return acc / n
    assert len(vectors) <= 64
    slots = [v.astype(np.float32) for v in vectors] + [np.zeros_like(vectors[0], dtype=np.float32)] * (64 - len(vectors))
    w = 1
    while w < 64:
        for k in range(0, 64 - w, 2 * w):
            slots[k] = slots[k] + slots[k + w]
        w *= 2
    return slots[0] / n


def ref_sync(base, subs, part, tree=False):
    """The base after a sync of every site's sub-model; the last bias is the site mean."""
    last = len(base) - 1
    new = [(W.copy(), b.copy()) for W, b in base]
    for s, sub in enumerate(subs):
        for k, ((W, b), (rows, cols)) in enumerate(zip(new, _blocks(len(base), part, s))):
            r = rows if rows is not None else np.arange(W.shape[0])
            c = cols if cols is not None else np.arange(W.shape[1])
            W[np.ix_(r, c)] = sub[k][0]
            if k < last:
                b[cols] = sub[k][1]
    new[last] = (new[last][0], site_mean([sub[last][1] for sub in subs], tree))
    return new


def coverage(base, part, S):
    """How often each cell of every base tensor but the shared bias is written by a sync: [(W counts, b counts)]."""
    last = len(base) - 1
    out = []
    for k, (W, b) in enumerate(base):
        cw, cb = np.zeros(W.shape, np.int64), np.zeros(b.shape, np.int64)
        for s in range(S):
            rows, cols = _blocks(len(base), part, s)[k]
            r = rows if rows is not None else np.arange(W.shape[0])
            c = cols if cols is not None else np.arange(W.shape[1])
            cw[np.ix_(r, c)] += 1
            if k < last:
                cb[cols] += 1
        out.append((cw, cb))
    return out


def perturbed(sub, site, scale=0.05):
    """What perturb(model, site) makes of a sub-model given as layers (float32 arithmetic, parameter order)."""
    gen = torch.Generator().manual_seed(1000 + site)
    out = []
    for layer in sub:
        new = []
        for t in layer:
            v = torch.from_numpy(np.ascontiguousarray(t)).float()
            v = v + (torch.rand(v.shape, generator=gen, dtype=torch.float32) - 0.5) * scale
            new.append(v.numpy())
        out.append(tuple(new))
    return out


def arena_layers(arena):
    """[(W, b)] float32 read from a gist_amd.arena.BaselineGCNArena."""
    return [tuple(np.asarray(t, dtype=np.float32) for t in layer) for layer in arena.export()]


def flat_layers(arena, flat):
    """The same, read from `flat`, a flat tensor in the arena's layout (one site's part of `gathered`)."""
    return [tuple(t.detach().cpu().numpy().copy() for t in arena.layer_views(flat, k)) for k in range(len(arena.dims))]


def base_init_for(dims, seed):
    """Full-width initial parameters per layer (W [in, out], b), the same on every rank."""
    gen = torch.Generator().manual_seed(seed)

    def r(*shape):
        return (torch.rand(*shape, generator=gen) - 0.5) * 0.4
    return [(r(i, o), r(o)) for (i, o) in dims]


def compare(got, want, what, errs):
    """Every tensor of `got` equals `want` bit for bit."""
    if len(got) != len(want):
        errs.append('%s: %d layers, want %d' % (what, len(got), len(want)))
        return
    for k, (gl, wl) in enumerate(zip(got, want)):
        for name, gt, wt in zip(('W', 'b'), gl, wl):
            if gt.shape != wt.shape:
                errs.append('%s: layer %d %s shape %s, want %s' % (what, k, name, gt.shape, wt.shape))
            elif gt.dtype != np.float32 or wt.dtype != np.float32 or gt.tobytes() != wt.tobytes():
                errs.append('%s: layer %d %s' % (what, k, name))


def check_round(ws, S, H, L, base_init, seed, all_base, tree=False, after=None):
    """Initial dispatch, perturbed sub-models, sync, re-dispatch, perturbed again, sync on the wrappers `ws` of this
    process (one per process under a process group, or all S sites on a LocalCommGroup), each step bit for bit against
    the restatement.  `all_base()` returns every rank's base arena (flat) for the cross-rank check; tree: the summation
    order of the movers in use (site_mean); `after(what)` is called after every dispatch and sync.  Returns a list of
    failures."""
    errs = []
    local = len(ws) > 1
    after = after if after is not None else (lambda what: None)
    base0 = [tuple(t.float().numpy() for t in layer) for layer in base_init]

    def draw(sd):
        random.seed(sd)
        want = ref_sample(S, H, L)
        want_state = random.getstate()
        random.seed(sd)
        return want, want_state

    def check_partition(w, want, want_state, what):
        if random.getstate() != want_state:
            errs.append('%s: python random consumed differently from %d shuffles of range(%d)' % (what, L, H))
        for k in range(L):
            for s in range(S):
                if not np.array_equal(w.current_partition[k][s][0].numpy(), want[k][s][0]):
                    errs.append('%s: partition %d site %d' % (what, k, s))

    def both_sync():
        for w in ws:
            w.sync_gather()
        for w in ws:
            w.sync_apply()

    def check_sync(base_before, subs, want, what):
        base_after = ref_sync(base_before, subs, want, tree)
        for w in ws:
            got = arena_layers(w.base)
            compare(got, base_after, '%s base rank %d' % (what, w.rank), errs)
            if not torch.equal(w.sub.b[-1].cpu(), w.base.b[-1].cpu()):
                errs.append('%s rank %d: the shared bias of the sub-model is not the base one' % (what, w.rank))
            if w.base_model is not None:
                model = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in w.base_model.layers]
                compare(model, got, '%s base_model rank %d' % (what, w.rank), errs)
            for s in range(S):          # what the collective brought: every site's sub arena as it stood
                P = w.sub.numel
                compare(flat_layers(w.sub, w.gathered[s * P:(s + 1) * P]), subs[s], '%s gathered rank %d site %d'
                        % (what, w.rank, s), errs)
        flats = [b.detach().cpu() for b in all_base()]
        if not all(torch.equal(f, flats[0]) for f in flats):
            errs.append('%s: the base replicas differ between the ranks' % what)
        # no cell of the base is written twice.  The first and the last weight and every hidden bias are covered exactly
        # once; of a middle weight [H, H] the sites own the S blocks (idx_k-1, idx_k) -- H * H / S cells -- and every cell
        # outside them keeps the bits it had before the sync
        n_layers = len(base_before)
        for k, (cw, cb) in enumerate(coverage(base_before, want, S)):
            middle = 0 < k < n_layers - 1
            if cw.max() > 1 or (not middle and not (cw == 1).all()) or (middle and cw.sum() * S != cw.size):
                errs.append('%s: the blocks of layer %d\'s weight: counts %s' % (what, k, np.unique(cw).tolist()))
            if k < n_layers - 1 and not (cb == 1).all():
                errs.append('%s: the blocks of layer %d\'s bias do not cover it exactly once' % (what, k))
            for w in ws:
                got = w.base.W[k].detach().cpu().numpy()
                if got[cw == 0].tobytes() != base_before[k][0][cw == 0].tobytes():
                    errs.append('%s rank %d: layer %d: a cell outside every site\'s block changed' % (what, w.rank, k))
        return base_after

    # the initial dispatch
    want, want_state = draw(seed)
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.ini_sync_dispatch_model(part)
    after('ini dispatch')
    for w in ws:
        check_partition(w, want, want_state, 'ini rank %d' % w.rank)
        compare(arena_layers(w.base), base0, 'replica rank %d' % w.rank, errs)
        compare(arena_layers(w.sub), ref_dispatch(base0, want, w.rank), 'ini sub rank %d' % w.rank, errs)
    # every site 'trains', then the sync
    for w in ws:
        perturb(w.sub_model, w.rank)
    both_sync()
    after('sync')
    subs = [perturbed(ref_dispatch(base0, want, s), s) for s in range(S)]
    base1 = check_sync(base0, subs, want, 'sync')
    # a re-dispatch on a new partition, training again, the second sync
    want, want_state = draw(seed + 1)
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.dispatch_model(part)
    after('dispatch')
    for w in ws:
        check_partition(w, want, want_state, 'dispatch rank %d' % w.rank)
        compare(arena_layers(w.sub), ref_dispatch(base1, want, w.rank), 'sub rank %d' % w.rank, errs)
    for w in ws:
        perturb(w.sub_model, 7 + w.rank)
    both_sync()
    after('second sync')
    subs = [perturbed(ref_dispatch(base1, want, s), 7 + s) for s in range(S)]
    check_sync(base1, subs, want, 'second sync')
    return errs
