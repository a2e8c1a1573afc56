"""TEST INFRASTRUCTURE (not product) for the GIST-for-GraphSAGE tests: a numpy float64 restatement of the split table of
gist_amd.ist.DistributedGraphSAGEWrapper -- the reference's GCN dispatch / sync (cluster_gcn_ist_distrib.py:100-367) with
the LayerNorm vectors following the bias -- and a check_round over it.  A model is [(W, b, gamma, beta)] per layer, the
output layer (W, b).  TorchBlocks, ref_sample and perturb are tests/gat_ist_restatement.py's."""
import random

import numpy as np
import torch

from tests.gat_ist_restatement import TorchBlocks, perturb, ref_sample        # noqa: F401  (re-exported)


def ref_dispatch(base, part, site):
    """The sub-model of `site` sliced from `base`."""
    last = len(base) - 1
    sub = []
    for k, layer in enumerate(base):
        W = layer[0]
        if k == 0:
            idx = part[0][site][0]
            sub.append((W[idx, :],) + tuple(v[idx] for v in layer[1:]))
        elif k == last:
            full = part[k - 1][site][1]
            sub.append((W[:, full], layer[1].copy()))
        else:
            idx, full = part[k][site][0], part[k - 1][site][1]
            sub.append((W[:, full][idx, :],) + tuple(v[idx] for v in layer[1:]))
    return sub


def ref_sync(base, subs, part):
    """The base after a sync of every site's sub-model; the last bias is the site mean."""
    last = len(base) - 1
    new = [tuple(t.copy() for t in layer) for layer in base]
    for s, sub in enumerate(subs):
        for k, layer in enumerate(new):
            W = layer[0]
            if k == 0:
                idx = part[0][s][0]
                W[idx, :] = sub[k][0]
                for v, sv in zip(layer[1:], sub[k][1:]):
                    v[idx] = sv
            elif k == last:
                full = part[k - 1][s][1]
                W[:, full] = sub[k][0]
            else:
                idx, full = part[k][s][0], part[k - 1][s][1]
                W[np.ix_(idx, full)] = sub[k][0]
                for v, sv in zip(layer[1:], sub[k][1:]):
                    v[idx] = sv
    mean = sum(sub[last][1] for sub in subs) / len(subs)
    new[last] = (new[last][0], mean)
    return new


def perturbed(sub, site, scale=0.05):
    """What perturb(model, site) makes of a sub-model given as layers (float32 arithmetic, parameter order)."""
    gen = torch.Generator().manual_seed(1000 + site)
    out = []
    for layer in sub:
        new = []
        for t in layer:
            v = torch.from_numpy(np.ascontiguousarray(t)).float()
            v = v + (torch.rand(v.shape, generator=gen, dtype=torch.float32) - 0.5) * scale
            new.append(v.double().numpy())
        out.append(tuple(new))
    return out


def layers_of(model):
    """A gist_amd.modules.GraphSAGE as float64 layers."""
    out = []
    for layer in model.layers:
        group = [layer.linear.weight, layer.linear.bias]
        if isinstance(layer.lynorm, torch.nn.LayerNorm):
            group += [layer.lynorm.weight, layer.lynorm.bias]
        out.append(tuple(t.detach().cpu().double().numpy().copy() for t in group))
    return out


def arena_layers(arena):
    """The same, read from a gist_amd.arena.GraphSAGEArena."""
    return [tuple(np.asarray(t, dtype=np.float64) for t in layer) for layer in arena.export()]


def base_init_for(dims, seed):
    """Full-width initial parameters per layer (W, b, gamma, beta) -- (W, b) last --, the same on every rank."""
    gen = torch.Generator().manual_seed(seed)

    def r(*shape):
        return (torch.rand(*shape, generator=gen) - 0.5) * 0.4
    last = len(dims) - 1
    return [(r(o, 2 * i), r(o)) + ((1.0 + r(o), r(o)) if k < last else ()) for k, (i, o) in enumerate(dims)]


def compare(got, want, what, errs, tol_last_bias=0.0):
    """Every tensor of `got` equals `want` exactly (the moves are copies); the last bias within tol."""
    last = len(want) - 1
    if len(got) != len(want):
        errs.append('%s: %d layers, want %d' % (what, len(got), len(want)))
        return
    for k, (gl, wl) in enumerate(zip(got, want)):
        if len(gl) != len(wl):
            errs.append('%s: layer %d has %d tensors, want %d' % (what, k, len(gl), len(wl)))
            continue
        for j, (gt, wt) in enumerate(zip(gl, wl)):
            if gt.shape != wt.shape:
                errs.append('%s: layer %d tensor %d shape %s, want %s' % (what, k, j, gt.shape, wt.shape))
            elif k == last and j == 1 and tol_last_bias:
                if np.abs(gt - wt).max() > tol_last_bias:
                    errs.append('%s: shared bias off by %g > %g' % (what, np.abs(gt - wt).max(), tol_last_bias))
            elif not np.array_equal(gt, wt):
                errs.append('%s: layer %d tensor %d' % (what, k, j))


def check_round(ws, S, H, L, base_init, seed, all_base, after=None):
    """Initial dispatch, perturbed sub-models, sync, re-dispatch, sync without training on the wrappers `ws` of this
    process (one per process under a process group, or all S sites on a LocalCommGroup), each step against the float64
    restatement.  `all_base()` returns every rank's base arena (flat) for the bitwise cross-rank check; `after(what)` is
    called after every dispatch and sync.  The shared bias is held to 4 * 2^-24 * max |b|: S - 1 <= 3 additions and a
    division at S <= 4.  Returns a list of failures."""
    errs = []
    local = len(ws) > 1
    after = after if after is not None else (lambda what: None)
    base0 = [tuple(t.double().numpy() for t in layer) for layer in base_init]

    def draw():
        random.seed(seed)
        want = ref_sample(S, H, L)
        want_state = random.getstate()
        random.seed(seed)
        return want, want_state

    def check_partition(w, want, want_state, what):
        if random.getstate() != want_state:
            errs.append('%s: python random consumed differently from %d shuffles of range(%d)' % (what, L, H))
        for k in range(L):
            for s in range(S):
                if not np.array_equal(w.current_partition[k][s][0].numpy(), want[k][s][0]) or \
                        not np.array_equal(w.current_partition[k][s][1].numpy(), want[k][s][1]):
                    errs.append('%s: partition %d site %d' % (what, k, s))

    def both_sync():
        for w in ws:
            w.sync_gather()
        for w in ws:
            w.sync_apply()

    # the initial dispatch
    want, want_state = draw()
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.ini_sync_dispatch_model(part)
    after('ini dispatch')
    for w in ws:
        check_partition(w, want, want_state, 'ini rank %d' % w.rank)
        compare(arena_layers(w.base), base0, 'replica rank %d' % w.rank, errs)
        compare(layers_of(w.sub_model), ref_dispatch(base0, want, w.rank), 'ini sub rank %d' % w.rank, errs)
    # every site 'trains', then the sync
    for w in ws:
        perturb(w.sub_model, w.rank)
    both_sync()
    after('sync')
    subs = [perturbed(ref_dispatch(base0, want, s), s) for s in range(S)]
    base1 = ref_sync(base0, subs, want)
    tol = 4.0 * 2.0 ** -24 * max(float(np.abs(sub[-1][1]).max()) for sub in subs)
    for w in ws:
        got = arena_layers(w.base)
        compare(got, base1, 'sync base rank %d' % w.rank, errs, tol_last_bias=tol)
        if not torch.equal(w.sub.b[-1].cpu(), w.base.b[-1].cpu()):
            errs.append('rank %d: the shared bias of the sub-model is not the base one' % w.rank)
        if w.base_model is not None:
            compare(layers_of(w.base_model), got, 'base_model rank %d' % w.rank, errs)
    flats = [b.detach().cpu() for b in all_base()]
    if not all(torch.equal(f, flats[0]) for f in flats):
        errs.append('the base replicas differ between the ranks after a sync')
    # a re-dispatch, then a sync without training: the identity
    want, want_state = draw()
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.dispatch_model(part)
    after('dispatch')
    for w in ws:
        check_partition(w, want, want_state, 'dispatch rank %d' % w.rank)
        compare(layers_of(w.sub_model), ref_dispatch(arena_layers(w.base), want, w.rank), 'sub rank %d' % w.rank, errs)
    before = [w.base.params.clone() for w in ws]
    both_sync()
    after('sync again')
    for w, b in zip(ws, before):
        if not torch.equal(w.base.params, b):
            errs.append('rank %d: dispatch -> sync without training changed the base' % w.rank)
    return errs
