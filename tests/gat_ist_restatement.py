"""TEST INFRASTRUCTURE (not product) for the GIST-for-GAT tests: a float64 restatement of the reference's per-head
dispatch / sync loops (cluster_gcn_ist_distrib_gat.py:96-205,302-391) under the readings of DESIGN.md §9 (every loop
over the layer's own heads; boundary k takes partition k; the last layer's attn vector is the site mean), its
create_partition (:51-65), and a torch-indexing double of gist_amd.ist.HipBlocks for the CPU."""
import random

import numpy as np
import torch


class TorchBlocks(object):
    """Test double for gist_amd.ist.HipBlocks (same contract as gist_block_gather/scatter_f32 and gist_mean_rows_f32)."""

    def gather(self, src, row_idx, col_idx, dst):
        s = src
        if row_idx is not None:
            s = s[row_idx.long()]
        if col_idx is not None:
            s = s[:, col_idx.long()]
        dst.copy_(s)

    def scatter(self, src, row_idx, col_idx, dst):
        r = row_idx.long() if row_idx is not None else torch.arange(src.shape[0])
        c = col_idx.long() if col_idx is not None else torch.arange(src.shape[1])
        dst[r[:, None], c[None, :]] = src

    def mean_rows(self, src_flat, stride, n_src, n, out):
        acc = torch.zeros(n)
        for s in range(n_src):
            acc = acc + src_flat[s * stride:s * stride + n]
        out.copy_(acc / n_src)


def ref_create_partition(num_subnet, size):
    """:51-65 as written: shuffle range(size), deal element i to site i % num_subnet."""
    possible = [x for x in range(size)]
    random.shuffle(possible)
    lists = [[] for _ in range(num_subnet)]
    for i in range(size):
        lists[i % num_subnet].append(possible[i])
    return [(np.array(l, dtype=np.int64), np.concatenate([l, np.array(l) + size]).astype(np.int64)) for l in lists]


def ref_sample(S, H, n_layers):
    """:85-90: n_layers partitions, whatever the layer count of the model."""
    return [ref_create_partition(S, H) for _ in range(n_layers)]


def heads_of(model):
    """[[ (fc float64 [O, I], attn float64 [1, 2O]) per head ] per layer] of a gist_amd.modules.GAT."""
    return [[(hd.fc.weight.detach().cpu().double().numpy().copy(), hd.attn_fc.weight.detach().cpu().double().numpy().copy())
             for hd in layer.heads] for layer in model.layers]


def heads_from_params(params, dims):
    """The same, from gist_amd.ist.gat_params() layout [(W [nh*O, I], A [nh, 2O])] with dims [(I, O, nh)]."""
    out = []
    for (W, A), (i, o, nh) in zip(params, dims):
        W = np.asarray(W, dtype=np.float64).reshape(nh * o, i)
        A = np.asarray(A, dtype=np.float64).reshape(nh, 2 * o)
        out.append([(W[h * o:(h + 1) * o].copy(), A[h:h + 1].copy()) for h in range(nh)])
    return out


def ref_dispatch(base, part, site):
    """The sub-model of `site` sliced from `base` (:302-391, per head)."""
    last = len(base) - 1
    sub = []
    for k, layer in enumerate(base):
        heads = []
        for fc, attn in layer:
            if k == 0:
                idx, full = part[0][site]
                heads.append((fc[idx, :], attn[:, full]))
            elif k == last:
                idx, _ = part[k - 1][site]
                heads.append((fc[:, idx], attn.copy()))
            else:
                prev, _ = part[k - 1][site]
                nxt, full = part[k][site]
                heads.append((fc[:, prev][nxt, :], attn[:, full]))
        sub.append(heads)
    return sub


def ref_sync(base, subs, part):
    """The base after a sync of every site's sub-model (:96-205, per head); the last attn is the site mean."""
    last = len(base) - 1
    new = [[(fc.copy(), attn.copy()) for fc, attn in layer] for layer in base]
    for s, sub in enumerate(subs):
        for k, layer in enumerate(new):
            for h, (fc, attn) in enumerate(layer):
                sfc, sattn = sub[k][h]
                if k == 0:
                    idx, full = part[0][s]
                    fc[idx, :] = sfc
                    attn[:, full] = sattn
                elif k == last:
                    idx, _ = part[k - 1][s]
                    fc[:, idx] = sfc
                else:
                    prev, _ = part[k - 1][s]
                    nxt, full = part[k][s]
                    rows = fc[:, prev]
                    rows[nxt, :] = sfc
                    fc[:, prev] = rows
                    attn[:, full] = sattn
    mean = sum(sub[last][0][1] for sub in subs) / len(subs)
    new[last][0] = (new[last][0][0], mean)
    return new


def perturb(model, site, scale=0.05):
    """'Training' of site `site`: add a site-seeded pattern to every parameter of its sub-model, in place."""
    gen = torch.Generator().manual_seed(1000 + site)
    with torch.no_grad():
        for p in model.parameters():
            p.add_((torch.rand(p.shape, generator=gen, dtype=torch.float32) - 0.5).to(p.device) * scale)


def compare(got, want, what, errs, tol_last_attn=0.0):
    """Per head, fc and attn of `got` equal `want` exactly (the moves are copies); the last attn within tol."""
    last = len(want) - 1
    if len(got) != len(want):
        errs.append('%s: %d layers, want %d' % (what, len(got), len(want)))
        return
    for k, (gl, wl) in enumerate(zip(got, want)):
        if len(gl) != len(wl):
            errs.append('%s: layer %d has %d heads, want %d' % (what, k, len(gl), len(wl)))
            continue
        for h, ((gf, ga), (wf, wa)) in enumerate(zip(gl, wl)):
            if gf.shape != wf.shape or not np.array_equal(gf, wf):
                errs.append('%s: layer %d head %d fc' % (what, k, h))
            tol = tol_last_attn if k == last else 0.0
            if ga.shape != wa.shape or (np.abs(ga - wa).max() > tol if tol else not np.array_equal(ga, wa)):
                errs.append('%s: layer %d head %d attn' % (what, k, h))


def arena_heads(arena):
    """heads_of() of a gist_amd.ist.GATArena, read from the arena itself."""
    return heads_from_params([(W.detach().cpu().numpy(), A.detach().cpu().numpy()) for W, A in zip(arena.W, arena.A)],
                             arena.dims)


def perturbed(sub, site, scale=0.05):
    """What perturb(model, site) makes of a sub-model given as heads (float32 arithmetic, parameter order)."""
    gen = torch.Generator().manual_seed(1000 + site)
    out = []
    for layer in sub:
        heads = []
        for fc, attn in layer:
            pair = []
            for t in (fc, attn):
                v = torch.from_numpy(np.ascontiguousarray(t)).float()
                v = v + (torch.rand(v.shape, generator=gen, dtype=torch.float32) - 0.5) * scale
                pair.append(v.double().numpy())
            heads.append(tuple(pair))
        out.append(heads)
    return out


def base_init_for(dims, seed):
    """Full-width initial parameters in gist_amd.ist.gat_params() layout, the same on every rank."""
    gen = torch.Generator().manual_seed(seed)
    return [((torch.rand(nh * o, i, generator=gen) - 0.5) * 0.4, (torch.rand(nh, 2 * o, generator=gen) - 0.5) * 0.4)
            for (i, o, nh) in dims]


def check_round(ws, S, H, L, base_init, seed, all_base, tol=1e-6):
    """Initial dispatch, perturbed sub-models, sync, re-dispatch, sync without training on the wrappers `ws` of this
    process (one per process under a process group, or all S sites on a LocalCommGroup), each step against the
    float64 restatement.  `all_base()` returns every rank's base arena (flat) for the bitwise cross-rank check.
    Returns a list of failures."""
    errs = []
    local = len(ws) > 1
    base_dims = ws[0].base_dims
    base0 = heads_from_params([(W.numpy(), A.numpy()) for W, A in base_init], base_dims)

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
                if not np.array_equal(w.current_partition[k][s][0].numpy(), want[k][s][0]):
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
    for w in ws:
        check_partition(w, want, want_state, 'ini rank %d' % w.rank)
        compare(arena_heads(w.base), base0, 'replica rank %d' % w.rank, errs)
        compare(heads_of(w.sub_model), ref_dispatch(base0, want, w.rank), 'ini sub rank %d' % w.rank, errs)
    # every site 'trains', then the sync
    for w in ws:
        perturb(w.sub_model, w.rank)
    both_sync()
    subs = [perturbed(ref_dispatch(base0, want, s), s) for s in range(S)]
    base1 = ref_sync(base0, subs, want)
    for w in ws:
        got = arena_heads(w.base)
        compare(got, base1, 'sync base rank %d' % w.rank, errs, tol_last_attn=tol)
        if not torch.equal(w.sub.A[-1].cpu(), w.base.A[-1].cpu()):
            errs.append('rank %d: the shared attn of the sub-model is not the base one' % w.rank)
        if w.base_model is not None:
            compare(heads_of(w.base_model), got, 'base_model rank %d' % w.rank, errs)
    flats = [b.detach().cpu() for b in all_base()]
    if not all(torch.equal(f, flats[0]) for f in flats):
        errs.append('the base replicas differ between the ranks after a sync')
    # a re-dispatch, then a sync without training: the identity
    want, want_state = draw()
    part = ws[0].sample_partitions() if local else None
    for w in ws:
        w.dispatch_model(part)
    for w in ws:
        check_partition(w, want, want_state, 'dispatch rank %d' % w.rank)
        compare(heads_of(w.sub_model), ref_dispatch(arena_heads(w.base), want, w.rank), 'sub rank %d' % w.rank, errs)
    before = [w.base.params.clone() for w in ws]
    both_sync()
    for w, b in zip(ws, before):
        if not torch.equal(w.base.params, b):
            errs.append('rank %d: dispatch -> sync without training changed the base' % w.rank)
    return errs
