#!/usr/bin/env python3
"""GIST for the BaselineGCN family (gist_amd.modules.BaselineGCN, cluster_gcn/modules.py:316-349: the plain GraphConv
stack of the Cluster-GCN and GIST papers) -- the CLI of cluster_gcn_ist_distrib.py (flags :520-559) and its output
contract (five result lines :475-479, or the results pickle with --save_results), one process per GPU, running on
gist_amd.ist.DistributedBaselineGCNWrapper and gist_amd.ist.train_baseline_gcn.

    for i in 0 1; do
      python -m gist_amd.scripts.cluster_gcn_ist_distrib_baseline --num_subnet 2 --rank $i --cuda-id $i \\
          --n-hidden 512 --n-layers 2 --dropout 0.2 --use_layernorm True --host-path step --dataset reddit-synth &
    done; wait

`--host-path module` (the default) is the reference's loop body on `ist_model.sub_model`; `--host-path step` runs every
iteration as one gist_baseline_gcn_step call on the wrapper's BaselineGCNEngine.  The family has no phase calls, so there
is no `--host-path phases`.  `--use_layernorm` is honoured: it is the reference's `type=bool` flag (any non-empty string
is True) and means the model's whole-tensor norm, which a sub-model takes over [n, H / S] and the base over [n, H].
`--use-pp` is refused: a GraphConv layer has no [X | A^X] input.  Rank 0's base model is evaluated by its own full-graph
forward.  Set-up (seeds, device, process group, --normalize, data loading) is cluster_gcn_ist_distrib's.
"""
import argparse
import os

import torch.distributed as dist

from gist_amd.scripts.cluster_gcn_ist_distrib import add_ist_args, setup


def build_parser():
    parser = add_ist_args(argparse.ArgumentParser(description='GCN'))
    parser.add_argument("--exp_name", type=str, default='distributed_gnn_ist')
    # (not a flag of the reference) gist_amd.ist.train_baseline_gcn's host_path
    parser.add_argument("--host-path", choices=['module', 'step'], default='module')
    return parser


def report(args, res, log=print):
    """With --save_results the pickle {total_time, trn_losses, val_accs, test_accs} goes to
    ./results/{exp_name}_result.pckl (returns its path); otherwise the five result lines (:475-479)."""
    from gist_amd import ist
    if args.save_results:
        import pickle
        os.makedirs('./results', exist_ok=True)
        path = os.path.join('./results', args.exp_name + '_result.pckl')
        with open(path, 'wb') as f:
            pickle.dump({'total_time': res['total_time'], 'trn_losses': res['trn_losses'],
                         'val_accs': res['val_accs'], 'test_accs': res['test_accs']}, f)
        return path
    ist.print_results(res, log=log)
    return None


def main(args=None, dataset=None, log=print, comm=None):
    """comm: the wrapper's collectives (None: gist_amd.ist.TorchDistComm over the process group set up here)."""
    from gist_amd import ist
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    if args is None:
        args = build_parser().parse_args()
    assert (args.n_hidden % args.num_subnet) == 0
    host_path = getattr(args, 'host_path', 'module')
    if args.use_pp:
        raise SystemExit('gist_amd: --use-pp is not offered for the BaselineGCN family (a GraphConv layer reads h alone, '
                         'there is no [X | A^X] input to precompute)')
    if args.cuda_id < 0:
        raise SystemExit('gist_amd: the BaselineGCN family runs on a GPU (--cuda-id >= 0)')
    device, data, g, in_feats, n_classes, train_nid, par_li, psize = setup(args, dataset, log)
    iter_cls = EngineClusterIter if host_path == 'step' else ClusterIter
    cluster_iterator = iter_cls(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li,
                                device=device)                                       # get_data (one shuffle)
    g = g.to(device)
    ist_model = ist.DistributedBaselineGCNWrapper(args, g, in_feats, n_classes, device, comm=comm, seed=args.rnd_seed)
    log(f'{args.rank}: start initial dispatch', flush=True)
    ist_model.ini_sync_dispatch_model()
    log(f'{args.rank}: finish initial dispatch', flush=True)
    res = ist.train_baseline_gcn(ist_model, args, g, cluster_iterator, g.ndata['label'], g.ndata['val_mask'],
                                 g.ndata['test_mask'], log=log, host_path=host_path)
    if args.rank == 0:
        path = report(args, res, log=log)
        if path is not None:
            res['results_path'] = path
    dist.destroy_process_group()
    res['model'] = ist_model
    return res


if __name__ == '__main__':
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    main()
