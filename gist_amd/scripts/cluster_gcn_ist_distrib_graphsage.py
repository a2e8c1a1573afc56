#!/usr/bin/env python3
"""GIST for the GraphSAGE family (gist_amd.modules.GraphSAGE, cluster_gcn/modules.py:100-189: the model the reference's
README names and --use-pp was written for) -- the CLI of cluster_gcn_ist_distrib.py (flags :520-559) and its output
contract (five result lines :475-479, or the results pickle with --save_results), one process per GPU, running on
gist_amd.ist.DistributedGraphSAGEWrapper and gist_amd.ist.train_graphsage.

    for i in 0 1; do
      python -m gist_amd.scripts.cluster_gcn_ist_distrib_graphsage --num_subnet 2 --rank $i --cuda-id $i \\
          --n-hidden 512 --n-layers 2 --dropout 0.2 --use-pp --host-path step --dataset reddit-synth &
    done; wait

`--host-path module` (the default) is the reference's loop body on `ist_model.sub_model`; `--host-path step` runs every
iteration as one gist_graphsage_step call on the wrapper's GraphSAGEEngine; `--host-path phases` keeps the loop body of
`module` and binds the sub-model to the iterator, so its forward, `loss.backward()` and `optimizer.step()` are the three
gist_graphsage_step_phase calls on that engine (bitwise `step`).  `--eval-path rows` evaluates rank 0's base
model with the row-blocked GraphSAGEFullGraphEvaluator instead of the model's own forward.  `--use-pp` is honoured: the
iterator's train features become [X | A^X] and layer 0 only projects them while training.  `--use_layernorm` is accepted:
this family's LayerNorm (with affine) is always on.  Set-up (seeds, device, process group, --normalize, data loading) is
cluster_gcn_ist_distrib's.
"""
import argparse
import os

import torch.distributed as dist

from gist_amd.scripts.cluster_gcn_ist_distrib import add_ist_args, setup


def build_parser():
    parser = add_ist_args(argparse.ArgumentParser(description='GCN'))
    parser.add_argument("--exp_name", type=str, default='distributed_gnn_ist')
    # (not flags of the reference) gist_amd.ist.train_graphsage's host_path and eval_path
    parser.add_argument("--host-path", choices=['step', 'module', 'phases'], default='module')
    parser.add_argument("--eval-path", choices=['layers', 'rows'], default='layers')
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
    if args.cuda_id < 0:
        raise SystemExit('gist_amd: the GraphSAGE family runs on a GPU (--cuda-id >= 0)')
    log('note: --use_layernorm %s: the GraphSAGE family\'s LayerNorm is always on (every layer but the output layer)'
        % args.use_layernorm, flush=True)
    device, data, g, in_feats, n_classes, train_nid, par_li, psize = setup(args, dataset, log)
    iter_cls = EngineClusterIter if host_path == 'step' else ClusterIter
    cluster_iterator = iter_cls(args.dataset, g, psize, args.batch_size, train_nid, use_pp=args.use_pp, par_li=par_li,
                                device=device)                                       # get_data (one shuffle)
    g = g.to(device)
    ist_model = ist.DistributedGraphSAGEWrapper(args, g, in_feats, n_classes, device, comm=comm, seed=args.rnd_seed)
    log(f'{args.rank}: start initial dispatch', flush=True)
    ist_model.ini_sync_dispatch_model()
    log(f'{args.rank}: finish initial dispatch', flush=True)
    res = ist.train_graphsage(ist_model, args, g, cluster_iterator, g.ndata['label'], g.ndata['val_mask'],
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
