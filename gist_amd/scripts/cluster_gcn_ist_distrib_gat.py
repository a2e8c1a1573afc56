#!/usr/bin/env python3
"""GIST for the GAT family -- CLI and output contract of the reference's cluster_gcn/cluster_gcn_ist_distrib_gat.py
(flags :538-580, four result lines or the results pickle :481-499), one process per GPU, running on the gist_amd HIP
path: gist_amd.ist.DistributedGATWrapper and gist_amd.ist.train_gat, the reference's loop on the drop-in classes.
`--host-path engine` (not a flag of the reference) runs every step as one gist_gat_step call on the wrapper's
GATEngine instead: the same numbers bit for bit, fewer launches.  `--host-path phases` keeps the reference's loop body and
binds `sub_model` to the iterator (gist_amd.module_engine.bind_gat): the engine's launches as three phase calls.

Launch like the reference's GAT sweep (script/reddit/run_gat_distrib_sweep.py): one process per rank,

    for i in 0 1; do
      python -m gist_amd.scripts.cluster_gcn_ist_distrib_gat --num_subnet 2 --rank $i --cuda-id $i \\
          --n-hidden 512 --n-layers 1 --n-heads 4 --lr 0.01 --n-epochs 40 --dataset reddit-synth &
    done; wait

Set-up (seeds, device, process group, --normalize, data loading) is cluster_gcn_ist_distrib's.  `--use_layernorm` and
`--dropout` are accepted and have no effect, as in the reference: its GAT has neither.  Readings of the reference
where it cannot run as written: DESIGN.md §9.
"""
import argparse
import os

import torch.distributed as dist

from gist_amd.scripts.cluster_gcn_ist_distrib import add_ist_args, setup


def build_parser():
    parser = add_ist_args(argparse.ArgumentParser(description='GCN'))
    parser.add_argument('--n-heads', type=int, default=4)
    # (not a flag of the reference) cat: the hidden layers concatenate their heads (its comment, modules.py:87-89)
    parser.add_argument('--head-merge', choices=['mean', 'cat'], default='mean')
    parser.add_argument("--exp_name", type=str, default='distributed_gnn_ist')
    # (not a flag of the reference) module: the reference's loop on ist_model.sub_model / base_model; engine: one
    # gist_gat_step per iteration; phases: the module loop with sub_model bound to the iterator, three
    # gist_gat_step_phase calls per iteration (gist_amd.ist.train_gat, host_path)
    parser.add_argument("--host-path", choices=['module', 'engine', 'phases'], default='module')
    # (not a flag of the reference) blocked: rank 0's evaluate(base_model, g, ...) runs gist_amd.gat_eval's
    # GATFullGraphEvaluator instead of the model's own forward (gist_amd.ist.train_gat, eval_path)
    parser.add_argument("--eval-path", choices=['layers', 'blocked'], default='layers')
    return parser


def report(args, res, log=print):
    """:481-499 -- with --save_results the pickle {total_time, trn_losses, val_accs, test_accs} goes to
    ./results/{exp_name}_result.pckl (returns its path); otherwise exactly four lines in the reference's order, which
    its sweep reads by position."""
    if args.save_results:
        import pickle
        os.makedirs('./results', exist_ok=True)
        path = os.path.join('./results', args.exp_name + '_result.pckl')
        with open(path, 'wb') as f:
            pickle.dump({'total_time': res['total_time'], 'trn_losses': res['trn_losses'],
                         'val_accs': res['val_accs'], 'test_accs': res['test_accs']}, f)
        return path
    log(f"Training Time: {res['total_time']:.4f}")
    log(f"Last Test: {res['test_accs'][-1]:.4f}")
    log(f"Best Test: {max(res['test_accs']):.4f}")
    log(f"Best Val: {max(res['val_accs']):.4f}")
    return None


def main(args=None, dataset=None, log=print):
    from gist_amd import ist
    from gist_amd.sampler import ClusterIter, EngineClusterIter
    if args is None:
        args = build_parser().parse_args()
    assert (args.n_hidden % args.num_subnet) == 0
    host_path = getattr(args, 'host_path', 'module')
    if host_path in ('engine', 'phases') and (args.use_pp or args.cuda_id < 0):
        raise SystemExit('gist_amd: --host-path %s is the fused GAT step: it runs on a GPU (--cuda-id >= 0) and '
                         'extracts its batches from the plain features (no --use-pp); use --host-path module'
                         % host_path)
    if args.use_pp:
        raise NotImplementedError(
            'gist_amd: --use-pp cannot work with the GAT in the reference either (the feature width doubles after '
            'in_feats was read)')
    device, data, g, in_feats, n_classes, train_nid, par_li, psize = setup(args, dataset, log)
    iter_cls = EngineClusterIter if host_path == 'engine' else ClusterIter
    cluster_iterator = iter_cls(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li,
                                device=device)                                       # get_data (one shuffle)
    g = g.to(device)
    ist_model = ist.DistributedGATWrapper(args, g, in_feats, n_classes, device, seed=args.rnd_seed)   # :609
    log(f'{args.rank}: start initial dispatch', flush=True)
    ist_model.ini_sync_dispatch_model()
    log(f'{args.rank}: finish initial dispatch', flush=True)
    if host_path == 'engine':
        cluster_iterator.bind(ist_model.attach_engine(cluster_iterator.n_max))
    res = ist.train_gat(ist_model, args, g, cluster_iterator, g.ndata['label'], g.ndata['val_mask'],
                        g.ndata['test_mask'], log=log, host_path=host_path,
                        eval_path=getattr(args, 'eval_path', 'layers'))
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
