"""GPU: GIST training of the small full-graph GCN (gist_amd/gcn_ist.py, scripts/gcn_train_ist.py) against a numpy GIST
loop written here from the reference's gcn/train_ist.py: dispatch by fancy indexing (:178-191), the learning-rate rule
(:193-198), merge by the reference's eight branches as they stand (:243-285, NOT through the product's one-rule plan), the
output bias that no branch writes back -- on oracle.gcn_oracle's forward / backward and gist_oracle's cross entropy and Adam.

Data: the 300-node graph of tests/golden/G5_train_ln1_L1.npz (60 feature columns, a multiple of 6), hidden 12, dropout 0,
5 epochs at iter_per_site = 2: dispatches in epochs 0, 2, 4 at lr, lr / 10, lr / 100 (int(2.5) = 2, int(3.75) = 3), merges
after epochs 1, 3 and 4 (the last one forced).  The partitions are teacher-forced."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4                         # tests/test_cora_gpu.py's, for the same kernels and run length
ACC_TOL = 0.011                    # its bar for argmax ties
EPS32 = float(np.finfo(np.float32).eps)
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'G5_train_ln1_L1.npz')
N_HIDDEN, N_EPOCHS, ITER_PER_SITE, LR, WD = 12, 5, 2, 0.01, 5e-4
_shared = {}


def golden():
    """(CitationDataset, oracle graph) of the fixture, built once."""
    if not _shared:
        from gist_amd.datasets import CitationDataset
        from oracle import gcn_oracle as G
        d = np.load(GOLD)
        f = d['feat'][:, :d['feat'].shape[1] // 6 * 6]
        data = CitationDataset('cora-mini', f, d['label'], d['train_mask'], d['val_mask'], d['test_mask'],
                               int(d['n_classes']), d['src'], d['dst'])
        n = f.shape[0]
        src, dst = G.with_self_loops(d['src'], d['dst'], n)
        _shared['v'] = (data, G.CitationGraph(src, dst, n))
    return _shared['v']


def make_init(in_feats, n_classes, L, seed):
    rs = np.random.RandomState(seed)
    dims = [(in_feats, N_HIDDEN)] + [(N_HIDDEN, N_HIDDEN)] * (L - 1) + [(N_HIDDEN, n_classes)]
    init = []
    for i, o in dims:
        a = np.sqrt(6.0 / (i + o))
        init.append((rs.uniform(-a, a, (i, o)).astype(np.float32), rs.uniform(-0.2, 0.2, o).astype(np.float32)))
    return init


def make_partitions(in_feats, L, S, si, so, seed, n_dispatch=3):
    rs = np.random.RandomState(seed)
    chunk = lambda n: tuple(torch.from_numpy(c.copy()) for c in np.split(rs.permutation(n), S))
    out = []
    for _ in range(n_dispatch):
        P = [chunk(in_feats) if si else None]
        P += [chunk(N_HIDDEN) for _ in range(1, L)]
        P.append(chunk(N_HIDDEN) if so else None)
        out.append(P)
    return out


def oracle_dispatch(main, P, s, L, si, so):
    """:176-191 for site s: the sub state dict, every tensor an owned array."""
    W, B = 'layers.%d.weight', 'layers.%d.bias'
    sub = {k: v.copy() for k, v in main.items()}
    if si:
        sub[W % 0] = main[W % 0][P[0][s], :]
    for i in range(1, L + 1):
        if i == L and not so:
            pass
        else:
            idx = P[i][s]
            sub[W % (i - 1)] = sub[W % (i - 1)][:, idx]
            sub[B % (i - 1)] = main[B % (i - 1)][idx]
            sub[W % i] = main[W % i][idx, :]
    return sub


def oracle_merge(main, subs, P, L, si, so):
    """:241-285, branch by branch; `main` is updated in place like the reference's update_dict / load_state_dict."""
    W, B = 'layers.%d.weight', 'layers.%d.bias'
    S = len(subs)
    mean = lambda key: (sum(sd[key] for sd in subs) / np.float32(S)).astype(np.float32)
    if si:
        if L <= 1 and not so:
            for idx, sd in zip(P[0], subs):
                main[W % 0][idx, :] = sd[W % 0]
        else:
            for i, sd in enumerate(subs):
                cur, nxt = P[0][i], P[1][i]
                rows = main[W % 0][cur, :]
                rows[:, nxt] = sd[W % 0]
                main[W % 0][cur, :] = rows
    else:
        if L <= 1 and not so:
            main[W % 0] = mean(W % 0)
        else:
            for i, sd in enumerate(subs):
                main[W % 0][:, P[1][i]] = sd[W % 0]
    for i in range(1, L + 1):
        if i == L:
            if not so:
                main[B % (i - 1)] = mean(B % (i - 1))
                main[W % i] = mean(W % i)
            else:
                for idx, sd in zip(P[i], subs):
                    main[B % (i - 1)][idx] = sd[B % (i - 1)]
                    main[W % i][idx, :] = sd[W % i]
        else:
            if i >= L - 1 and not so:
                for idx, sd in zip(P[i], subs):
                    main[B % (i - 1)][idx] = sd[B % (i - 1)]
                    main[W % i][idx, :] = sd[W % i]
            else:
                for j, sd in enumerate(subs):
                    cur, nxt = P[i][j], P[i + 1][j]
                    main[B % (i - 1)][cur] = sd[B % (i - 1)]
                    rows = main[W % i][cur, :]
                    rows[:, nxt] = sd[W % i]
                    main[W % i][cur, :] = rows


def oracle_loop(g, data, init, L, S, si, so, ln, parts):
    """The epochs of :140-299 in numpy: (site losses [epoch][site], records, the base after every merge)."""
    from oracle import gcn_oracle as G
    from oracle import gist_oracle as O
    W, B = 'layers.%d.weight', 'layers.%d.bias'
    main = {}
    for k, (w, b) in enumerate(init):
        main[W % k], main[B % k] = w.copy(), b.copy()
    parts = [[None if lv is None else [p.numpy() for p in lv] for lv in P] for P in parts]
    feats = np.asarray(data.features, np.float32)
    tmask = np.asarray(data.train_mask, bool)
    pairs = lambda sd: [(sd[W % k], sd[B % k]) for k in range(L + 1)]
    losses, record, merged = [], [], []
    for epoch in range(N_EPOCHS):
        if epoch % ITER_PER_SITE == 0:
            P = parts.pop(0)
            lr = LR
            if epoch >= int(N_EPOCHS * 0.5):
                lr /= 10
            if epoch >= int(N_EPOCHS * 0.75):
                lr /= 10
            subs = [oracle_dispatch(main, P, s, L, si, so) for s in range(S)]
            opts = [O.new_opt_state(pairs(sd)) for sd in subs]
        row = []
        for s in range(S):
            params = pairs(subs[s])
            x = feats[:, P[0][s]] if si else feats
            logits, caches = G.gcn_forward(g, x, params, ln)
            loss, dlog = O.cross_entropy(logits, data.labels, tmask)
            grads = G.gcn_backward(g, caches, dlog)
            opt = opts[s]
            opt['step'] += 1
            for k, ((w, b), (dw, db)) in enumerate(zip(params, grads)):
                O.adam_step(w, dw, opt['m'][k][0], opt['v'][k][0], opt['step'], lr, weight_decay=WD)
                O.adam_step(b, db, opt['m'][k][1], opt['v'][k][1], opt['step'], lr, weight_decay=WD)
            row.append(float(loss))
        losses.append(row)
        if (epoch + 1) % ITER_PER_SITE == 0 or epoch == N_EPOCHS - 1:
            oracle_merge(main, subs, P, L, si, so)
            merged.append({k: v.copy() for k, v in main.items()})
        ev, _ = G.gcn_forward(g, feats, pairs(main), ln)
        record.append((G.accuracy(ev, data.labels, data.val_mask), G.accuracy(ev, data.labels, data.test_mask)))
    return losses, record, merged


def state(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.named_parameters()}


def probe_class():
    from gist_amd.gcn_ist import GISTFullGraphTrainer

    class Probe(GISTFullGraphTrainer):
        """Records the base and the sub-models around every dispatch and merge of the real fit() loop."""
        events = None

        def dispatch(self, epoch, n_epochs, P=None):
            super().dispatch(epoch, n_epochs, P)
            self.events.append(('dispatch', epoch, state(self.model), [state(m) for m in self.sub_models],
                                [o.param_groups[0]['lr'] for o in self.optimizers], self.P))

        def merge(self):
            before = state(self.model)
            subs = [state(m) for m in self.sub_models]
            super().merge()
            self.events.append(('merge', None, before, subs, state(self.model), self.P))
    return Probe


def np_index(a, rows, cols):
    if rows is not None:
        a = a[rows]
    if cols is not None:
        a = a[..., cols]
    return a


CASES = list(itertools.product((2, 3), (1, 2, 3), (False, True), (False, True), (True, False)))


@pytest.mark.parametrize('S,L,si,so,ln', CASES)
def test_gist_loop_against_the_numpy_loop(S, L, si, so, ln):
    from gist_amd.gcn_ist import tensor_plan
    data, g = golden()
    in_feats = data.features.shape[1]
    init = make_init(in_feats, data.num_labels, L, seed=S * 10 + L)
    parts = make_partitions(in_feats, L, S, si, so, seed=S + 7 * L)
    t = probe_class()(data, N_HIDDEN, L, 0.0, ln, LR, WD, num_subnet=S, iter_per_site=ITER_PER_SITE, split_input=si,
                      split_output=so, init_params=init)
    t.events = []
    t.fit(N_EPOCHS, partitions=parts)
    want_losses, want_record, want_merged = oracle_loop(g, data, init, L, S, si, so, ln, parts)
    plan = tensor_plan(L, si, so)
    ev_d = [e for e in t.events if e[0] == 'dispatch']
    ev_m = [e for e in t.events if e[0] == 'merge']
    assert [e[1] for e in ev_d] == [0, 2, 4] and len(ev_m) == 3
    assert [e[4] for e in ev_d] == [[LR] * S, [LR / 10] * S, [LR / 10 / 10] * S]
    pick = lambda P, level, s: None if level is None else P[level][s].numpy()
    # every sub-model tensor right after a dispatch is numpy's indexing of the base, bit for bit
    for _, _, base, subs, _, P in ev_d:
        for s in range(S):
            for name, rows, cols, _ in plan:
                assert np.array_equal(subs[s][name], np_index(base[name], pick(P, rows, s), pick(P, cols, s))), name
    # after a merge: scattered parts are the sites' tensors bit for bit, averaged ones the float64 mean to S + 2 roundings
    for _, _, before, subs, after, P in ev_m:
        for name, rows, cols, how in plan:
            if how == 'scatter':
                for s in range(S):
                    assert np.array_equal(np_index(after[name], pick(P, rows, s), pick(P, cols, s)), subs[s][name]), name
            elif how == 'mean':
                stack = np.stack([sd[name].astype(np.float64) for sd in subs])
                bound = EPS32 * (S + 2) * np.abs(stack).mean(axis=0)
                assert (np.abs(after[name] - stack.mean(axis=0)) <= bound).all(), name
            else:
                assert np.array_equal(after[name], before[name]) and name == 'layers.%d.bias' % L
    # the loop against the numpy loop
    got_losses = np.array([[float(l.item()) for l in row] for row in t.site_losses])
    err_l = np.abs(got_losses - np.array(want_losses)).max()
    err_p = max(np.abs(t.merged[i][k][j] - want_merged[i][('layers.%d.weight', 'layers.%d.bias')[j] % k]).max()
                for i in range(3) for k in range(L + 1) for j in range(2))
    err_a = np.abs(np.array(t.history) - np.array(want_record)).max()
    print('gist S=%d L=%d si=%d so=%d ln=%d: loss %.2e params %.2e acc %.4f' % (S, L, si, so, ln, err_l, err_p, err_a))
    assert got_losses.shape == (N_EPOCHS, S) and len(t.merged) == 3
    assert err_l < TOL and err_p < TOL and err_a < ACC_TOL
    # the base keeps its INITIAL output bias (no branch of :243-285 names it)
    assert np.array_equal(state(t.model)['layers.%d.bias' % L], init[L][1])
    assert init[L][1].any()


def test_row_and_grid_norm_train_the_same_losses():
    """The same run with the sub-models' whole-tensor norm on the row kernel and on the grid kernels."""
    from gist_amd.gcn_ist import GISTFullGraphTrainer
    data, _ = golden()
    S, L = 2, 2
    init = make_init(data.features.shape[1], data.num_labels, L, seed=5)
    runs = {}
    for wn in ('row', 'grid'):
        t = GISTFullGraphTrainer(data, N_HIDDEN, L, 0.0, True, LR, WD, num_subnet=S, iter_per_site=ITER_PER_SITE,
                                 split_input=True, split_output=True, init_params=init, whole_norm=wn)
        assert all(m.whole_norm == wn for m in t.sub_models) and t.model.whole_norm == 'row'
        t.fit(N_EPOCHS, partitions=make_partitions(data.features.shape[1], L, S, True, True, seed=11))
        runs[wn] = np.array([[float(l.item()) for l in row] for row in t.site_losses])
    assert np.abs(runs['row'] - runs['grid']).max() < TOL


def test_cli_default_flags_on_cora_synth():
    """The reference's defaults (dropout 0.5, random projection, S = 2, split_input) through the script, 8 epochs."""
    from gist_amd.scripts import gcn_train_ist as cli
    args = cli.build_parser().parse_args(['--dataset', 'cora-synth', '--n-epochs', '8'])
    torch.manual_seed(0)
    np.random.seed(0)
    lines = []
    res = cli.main(args, log=lambda *a: lines.append(' '.join(map(str, a))))
    assert np.isfinite(np.array(res['site_losses'])).all() and np.array(res['site_losses']).shape == (8, 2)
    assert res['losses'][-1] < res['losses'][0]
    assert lines[0].startswith("----Data statistics------'") and '#Edges 10556' in lines[0]
    epochs = lines[1:9]
    keys = ['Epoch', 'Time(s)', 'Loss', 'Val Accuracy', 'Test Accuracy', 'ETputs(KTEPS)']
    for e, l in enumerate(epochs):
        fields = [f.strip() for f in l.split('|')]
        assert [' '.join(f.split()[:-1]) for f in fields] == keys, l
        assert fields[0] == 'Epoch %05d' % e
        assert ('nan' in fields[1]) == (e < 3)                      # np.mean([]) before the fourth epoch
    assert [l.split(':')[0] for l in lines[-3:]] == ['Final Test Accuracy', 'Best Val Accuracy', 'Best Test Accuracy']
    assert res['epoch_time'] > 0 and len(res['merged']) == 2 and len(res['record']) == 8
    assert res['model'].layers[0].weight.shape == (1432, 16)       # 1433 // 2 * 2 projected columns
