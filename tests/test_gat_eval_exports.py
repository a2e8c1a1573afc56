"""CPU: the full-graph GAT evaluation entries (gist_gat_row_stats_f32, gist_gat_aggregate_blocks_f32) are exported and
bound, refuse bad arguments before any launch, and GATFullGraphEvaluator refuses bad node blocks before any device work."""
import ctypes

import numpy as np
import pytest
import torch

P = ctypes.c_void_p(16)         # a non-null pointer no refused call dereferences


def _stats(L, rowptr=P, col=P, s_src=P, s_dst=P, n=4, heads=2, M=P, Lp=P):
    return L.gist_gat_row_stats_f32(rowptr, col, s_src, s_dst, n, heads, M, Lp, None)


def _blocks(L, rowptr=P, col=P, block_ptr=P, n_blocks=1, Z=P, ldz=16, s_src=P, s_dst=P, M=P, Lp=P, n=4, heads=2,
            out_dim=8, elu=1, cat=0, out=P, ldo=8):
    return L.gist_gat_aggregate_blocks_f32(rowptr, col, block_ptr, n_blocks, Z, ldz, s_src, s_dst, M, Lp, n, heads,
                                           out_dim, elu, cat, out, ldo, None)


def test_exported_and_bound():
    from gist_amd import _lib, gat_eval, hip
    L = _lib.load()
    for name in ('gist_gat_row_stats_f32', 'gist_gat_aggregate_blocks_f32'):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.gist_abi_version() == 16                      # additive: the ABI version stays
    assert hasattr(hip, 'gat_row_stats') and hasattr(hip, 'gat_aggregate_blocks')
    assert hasattr(gat_eval, 'GATFullGraphEvaluator')


def test_bad_sizes_return_einval_with_a_message():
    from gist_amd import _lib
    L = _lib.load()
    for kw in (dict(n=-1), dict(heads=0), dict(n=1 << 31)):
        assert _stats(L, **kw) == -1
        assert b'gist_gat_row_stats_f32: bad sizes' in L.gist_last_error()
    for kw in (dict(n=-1), dict(heads=0), dict(out_dim=0), dict(ldz=15), dict(ldo=7), dict(cat=1, ldo=15),
               dict(n_blocks=0), dict(n_blocks=-1), dict(n_blocks=5), dict(n=129, n_blocks=1)):
        assert _blocks(L, **kw) == -1, kw
        assert b'gist_gat_aggregate_blocks_f32: bad sizes' in L.gist_last_error()


def test_null_pointers_are_refused():
    from gist_amd import _lib
    L = _lib.load()
    for name in ('rowptr', 's_src', 's_dst', 'M', 'Lp'):
        assert _stats(L, **{name: None}) == -1
        assert b'gist_gat_row_stats_f32: null pointer' in L.gist_last_error()
    for name in ('rowptr', 'block_ptr', 'Z', 's_src', 's_dst', 'M', 'Lp', 'out'):
        assert _blocks(L, **{name: None}) == -1, name
        assert b'gist_gat_aggregate_blocks_f32: null pointer' in L.gist_last_error()


def test_no_rows_is_ok_and_touches_nothing():
    from gist_amd import _lib
    L = _lib.load()
    assert _stats(L, None, None, None, None, 0, 3, None, None) == 0
    assert _blocks(L, rowptr=None, col=None, block_ptr=None, n_blocks=0, Z=None, s_src=None, s_dst=None, M=None,
                   Lp=None, n=0, out=None) == 0


def _host_graph(n=300):
    from gist_amd.graph import Graph
    g = Graph.from_edges(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), n)
    g.ndata['feat'] = torch.zeros(n, 6)
    g.ndata['label'] = torch.zeros(n, dtype=torch.int64)
    return g


@pytest.mark.parametrize('bounds', [[0, 100, 100, 300], [0, 120, 110, 300], [0, 100, 200], [1, 100, 200, 300],
                                    [0, 129, 200, 300], [0]])
def test_evaluator_refuses_bad_node_blocks_before_any_device_work(bounds):
    """A host graph and device 'cuda': a constructor that allocated or moved anything first would fail differently on
    a machine without a GPU."""
    from gist_amd.gat_eval import GATFullGraphEvaluator
    g = _host_graph()
    dims = [(6, 8, 2), (8, 3, 1)]
    with pytest.raises(ValueError, match='node_blocks must be increasing boundaries 0..N of blocks of 1..128 nodes'):
        GATFullGraphEvaluator(g, dims, None, torch.device('cuda', 0), node_blocks=bounds)
    g.node_blocks = np.asarray(bounds, np.int64)          # ... and the graph's own boundaries likewise
    with pytest.raises(ValueError, match='node_blocks must be increasing'):
        GATFullGraphEvaluator(g, dims, None, torch.device('cuda', 0))


def test_cli_flag_and_train_gat_argument():
    from gist_amd.scripts import cluster_gcn, cluster_gcn_ist_distrib_gat
    import inspect
    from gist_amd import ist
    for mod in (cluster_gcn, cluster_gcn_ist_distrib_gat):
        p = mod.build_parser()
        assert p.parse_args([]).eval_path == 'layers'
        assert p.parse_args(['--eval-path', 'blocked']).eval_path == 'blocked'
    assert inspect.signature(ist.train_gat).parameters['eval_path'].default == 'layers'
