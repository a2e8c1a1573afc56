"""CPU: GIST for the small full-graph GCN (gist_amd/gcn_ist.py, scripts/gcn_train_ist.py) -- the parser against the
reference's gcn/train_ist.py:311-338, the partition draws against :150-166, the per-tensor dispatch / merge plan against a
table restated by hand from :178-191 and :243-285, and the new whole-tensor LayerNorm entry points of the C ABI."""
import ctypes
import itertools

import pytest
import torch

P16 = ctypes.c_void_p(16)         # a non-null, 16-byte aligned pointer no refused call dereferences


# -- the command line -----------------------------------------------------------------------------------------------
def test_parser_defaults_are_the_references():
    from gist_amd.scripts import gcn_train_ist as cli
    d = cli.build_parser().parse_args([])
    assert (d.dataset, d.use_ist, d.iter_per_site, d.num_subnet, d.dropout, d.split_output, d.split_input, d.gpu, d.lr,
            d.n_epochs, d.n_hidden, d.n_layers, d.weight_decay, d.self_loop, d.use_layernorm, d.use_random_proj) == (
        'cora', 'True', 5, 2, 0.5, 'False', 'True', 1, 0.01, 200, 16, 1, 5e-4, 'True', 'True', 'True')
    assert d.data_root is None
    assert all(v is True or v is False for v in cli.string_flags(d).values())
    assert cli.string_flags(d) == dict(use_ist=True, split_input=True, split_output=False, self_loop=True,
                                       use_layernorm=True, use_random_proj=True)


@pytest.mark.parametrize('name', ['use_ist', 'split_input', 'split_output', 'self_loop', 'use_layernorm',
                                  'use_random_proj'])
@pytest.mark.parametrize('bad', ['true', '1', 'yes', ''])
def test_a_bad_string_boolean_asserts(name, bad):
    from gist_amd.scripts import gcn_train_ist as cli
    d = cli.build_parser().parse_args([])
    setattr(d, name, bad)
    with pytest.raises(AssertionError, match='Only True or False for %s' % name):
        cli.main(d)


def test_shape_assert_bad_dataset_and_use_ist_false():
    from gist_amd.scripts import gcn_train_ist as cli
    parse = cli.build_parser().parse_args
    with pytest.raises(AssertionError):                                  # :62
        cli.main(parse(['--n-hidden', '16', '--num_subnet', '3']))
    with pytest.raises(NotImplementedError, match='reddit is not a valid dataset'):      # :69
        cli.main(parse(['--dataset', 'reddit']))
    with pytest.raises(FileNotFoundError):                               # the real files are not here: never a stand-in
        cli.main(parse(['--dataset', 'cora']))
    with pytest.raises(NotImplementedError, match='Should train with IST'):              # :289
        cli.main(parse(['--dataset', 'cora-synth', '--use_ist', 'False']))


def test_mean_of_nothing_is_nan_without_a_warning():
    import math
    import warnings
    from gist_amd.scripts import gcn_train_ist as cli
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert math.isnan(cli._mean([]))
    assert cli._mean([1.0, 3.0]) == 2.0


# -- partitions -----------------------------------------------------------------------------------------------------
COMBOS = list(itertools.product((False, True), (False, True)))


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('split_input,split_output', COMBOS)
@pytest.mark.parametrize('S', [2, 3])
def test_draw_partitions_shapes_partition_and_order(n_layers, split_input, split_output, S):
    from gist_amd.gcn_ist import draw_partitions
    in_feats, n_hidden = 30, 12
    torch.manual_seed(7 + n_layers)
    P = draw_partitions(in_feats, n_hidden, n_layers, S, split_input, split_output)
    assert len(P) == n_layers + 1
    assert (P[0] is not None) == split_input and (P[n_layers] is not None) == split_output
    for i, level in enumerate(P):
        if level is None:
            continue
        rng = in_feats if i == 0 else n_hidden
        assert len(level) == S and all(p.numel() == rng // S for p in level)
        assert sorted(torch.cat(list(level)).tolist()) == list(range(rng))
    assert all(P[i] is not None for i in range(1, n_layers))
    # the same calls by hand, in the reference's order (:150-166)
    torch.manual_seed(7 + n_layers)
    want = [torch.chunk(torch.randperm(in_feats), S) if split_input else None]
    for _ in range(1, n_layers):
        want.append(torch.chunk(torch.randperm(n_hidden), S))
    want.append(torch.chunk(torch.randperm(n_hidden), S) if split_output else None)
    for got, ref in zip(P, want):
        assert (got is None) == (ref is None)
        if got is not None:
            assert all(torch.equal(a, b) for a, b in zip(got, ref))


# -- the per-tensor plan --------------------------------------------------------------------------------------------
# (rows, cols, merge) per tensor, restated from train_ist.py.  Dispatch :178-191: W0 takes rows P[0] with split_input; for
# i = 1..L, unless i == L without split_output, W_{i-1} takes columns P[i], b_{i-1} entries P[i], W_i rows P[i].  Merge
# :243-285: 'S' = written back through index lists, 'M' = sum over sites / S, 'K' = no branch writes it (b_L).
W, B = 'layers.%d.weight', 'layers.%d.bias'
TABLE = {
    # L = 1
    (1, False, False): [(W % 0, None, None, 'M'), (B % 0, None, None, 'M'), (W % 1, None, None, 'M'), (B % 1, None, None, 'K')],
    (1, False, True): [(W % 0, None, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, None, 'S'), (B % 1, None, None, 'K')],
    (1, True, False): [(W % 0, 0, None, 'S'), (B % 0, None, None, 'M'), (W % 1, None, None, 'M'), (B % 1, None, None, 'K')],
    (1, True, True): [(W % 0, 0, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, None, 'S'), (B % 1, None, None, 'K')],
    # L = 2
    (2, False, False): [(W % 0, None, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, None, 'S'), (B % 1, None, None, 'M'),
                        (W % 2, None, None, 'M'), (B % 2, None, None, 'K')],
    (2, False, True): [(W % 0, None, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                       (W % 2, 2, None, 'S'), (B % 2, None, None, 'K')],
    (2, True, False): [(W % 0, 0, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, None, 'S'), (B % 1, None, None, 'M'),
                       (W % 2, None, None, 'M'), (B % 2, None, None, 'K')],
    (2, True, True): [(W % 0, 0, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                      (W % 2, 2, None, 'S'), (B % 2, None, None, 'K')],
    # L = 3
    (3, False, False): [(W % 0, None, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                        (W % 2, 2, None, 'S'), (B % 2, None, None, 'M'), (W % 3, None, None, 'M'), (B % 3, None, None, 'K')],
    (3, False, True): [(W % 0, None, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                       (W % 2, 2, 3, 'S'), (B % 2, None, 3, 'S'), (W % 3, 3, None, 'S'), (B % 3, None, None, 'K')],
    (3, True, False): [(W % 0, 0, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                       (W % 2, 2, None, 'S'), (B % 2, None, None, 'M'), (W % 3, None, None, 'M'), (B % 3, None, None, 'K')],
    (3, True, True): [(W % 0, 0, 1, 'S'), (B % 0, None, 1, 'S'), (W % 1, 1, 2, 'S'), (B % 1, None, 2, 'S'),
                      (W % 2, 2, 3, 'S'), (B % 2, None, 3, 'S'), (W % 3, 3, None, 'S'), (B % 3, None, None, 'K')],
}


@pytest.mark.parametrize('case', sorted(TABLE))
def test_tensor_plan_matches_the_restated_table(case):
    from gist_amd.gcn import graphconv_dims
    from gist_amd.gcn_ist import tensor_plan
    n_layers, split_input, split_output = case
    names = {'S': 'scatter', 'M': 'mean', 'K': 'keep'}
    assert tensor_plan(n_layers, split_input, split_output) == [(n, r, c, names[m]) for n, r, c, m in TABLE[case]]
    # the plan's index lists produce the shapes gcn.GCN gives a sub-model (gcn.py:26-55)
    in_feats, n_hidden, n_classes, S = 30, 12, 5, 3
    dims = graphconv_dims(in_feats, n_hidden, n_classes, n_layers, split_input, split_output, S)
    full = graphconv_dims(in_feats, n_hidden, n_classes, n_layers, False, False, 1)
    width = [in_feats // S] + [n_hidden // S] * n_layers
    for name, rows, cols, _ in TABLE[case]:
        k = int(name.split('.')[1])
        if name.endswith('weight'):
            assert dims[k] == (full[k][0] if rows is None else width[rows], full[k][1] if cols is None else width[cols])
        else:
            assert dims[k][1] == (full[k][1] if cols is None else width[cols])


def test_site_lr_is_the_references_schedule():
    from gist_amd.gcn_ist import site_lr
    got = [site_lr(0.01, e, 5) for e in range(5)]                    # int(2.5) = 2, int(3.75) = 3
    assert got[:2] == [0.01, 0.01] and got[2] == 0.01 / 10 and got[3] == got[4] == 0.01 / 10 / 10


def test_gcn_takes_whole_norm_keyword_only():
    import inspect
    from gist_amd.gcn import GCN
    ps = list(inspect.signature(GCN.__init__).parameters.values())
    assert [p.name for p in ps[1:12]] == ['g', 'in_feats', 'n_hidden', 'n_classes', 'n_layers', 'activation',
                                          'dropout', 'use_layernorm', 'split_input', 'split_output', 'num_subnet']
    assert ps[12].name == 'whole_norm' and ps[12].kind is inspect.Parameter.KEYWORD_ONLY and ps[12].default == 'row'
    with pytest.raises(ValueError, match="whole_norm must be 'row' or 'grid'"):
        GCN(None, 4, 4, 2, 1, None, 0.0, whole_norm='chip')


# -- the C ABI --------------------------------------------------------------------------------------------------------
def _fwd(L, x=P16, yhat=P16, stats=P16, n=8, partials=P16):
    return L.gist_ln_all_fwd_f32(x, yhat, stats, n, 1e-5, partials, None)


def _bwd(L, g=P16, yhat=P16, stats=P16, dx=P16, n=8, partials=P16):
    return L.gist_ln_all_bwd_f32(g, yhat, stats, dx, n, partials, None)


def test_ln_all_exported_and_bound():
    from gist_amd import _lib, autograd, hip, ops
    L = _lib.load()
    for name in ('gist_ln_all_partials', 'gist_ln_all_fwd_f32', 'gist_ln_all_bwd_f32'):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert hasattr(hip, 'ln_all_fwd') and hasattr(hip, 'ln_all_bwd') and hasattr(autograd, 'layer_norm_all')
    for name in ('layer_norm_all', 'layer_norm_all_bwd'):
        assert name in ops.OPS and hasattr(torch.ops.gist, name)
    assert str(torch.ops.gist.layer_norm_all.default._schema) == 'gist::layer_norm_all(Tensor x) -> (Tensor, Tensor)'
    with pytest.raises(NotImplementedError):               # no CPU kernel
        torch.ops.gist.layer_norm_all(torch.ones(4, 4))


def test_ln_all_partials_is_a_function_of_n_with_a_cap():
    from gist_amd import _lib
    q = _lib.load().gist_ln_all_partials
    assert [q(n) for n in (-1, 0, 1, 4096, 4097, 1024 * 4096, 1024 * 4096 + 1, 1 << 32)] == [
        0, 0, 4, 4, 8, 4096, 4096, 4096]


def test_ln_all_refuses_bad_arguments_with_its_own_name():
    from gist_amd import _lib
    L = _lib.load()
    for call, name, ptrs in ((_fwd, b'gist_ln_all_fwd_f32', ('x', 'yhat', 'stats', 'partials')),
                             (_bwd, b'gist_ln_all_bwd_f32', ('g', 'yhat', 'stats', 'dx', 'partials'))):
        for p in ptrs:
            assert call(L, **{p: None}) == -1, p
            assert L.gist_last_error().startswith(name + b': null pointer')
        assert call(L, n=-1) == -1 and L.gist_last_error().startswith(name + b': negative size')
        for n in (1 << 33, 1 << 40):
            assert call(L, n=n) == -1 and L.gist_last_error().startswith(name + b': size >= 2^31 * 4')
        assert call(L, partials=ctypes.c_void_p(20)) == -1 and L.gist_last_error().startswith(name + b': misaligned')


def test_ln_all_of_nothing_is_ok_and_touches_nothing():
    from gist_amd import _lib
    L = _lib.load()
    assert L.gist_ln_all_fwd_f32(None, None, None, 0, 1e-5, None, None) == 0
    assert L.gist_ln_all_bwd_f32(None, None, None, None, 0, None, None) == 0
