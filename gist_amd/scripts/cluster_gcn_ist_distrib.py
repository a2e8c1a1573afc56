#!/usr/bin/env python3
"""GIST distributed training -- CLI and output contract of the reference's
cluster_gcn/cluster_gcn_ist_distrib.py (flags :520-564, five result lines :475-479), one
process per GPU over RCCL, running on the gist_amd HIP path.

Launch like the reference (script/reddit/run_ist_distrib.sh): one process per rank,

    for i in 0 1 2 3; do
      python -m gist_amd.scripts.cluster_gcn_ist_distrib --num_subnet 4 --rank $i --cuda-id $i \\
          --iter_per_site 100 --n-hidden 4096 --n-layers 2 --dropout 0.2 --use_layernorm True \\
          --lr 0.01 --n-epochs 40 --rnd-seed 0 --dataset reddit-synth &
    done; wait

`--use_layernorm` keeps the reference's `type=bool` quirk (:538): any non-empty string is True.

`--host-path module` (not a flag of the reference) runs the reference's own loop (:394-447) statement for statement
on the drop-in classes: `ist_model.sub_model`, gist_amd.nn.CrossEntropyLoss, a new gist_amd.optim.Adam at every
dispatch point, `evaluate(ist_model.base_model, ...)` on rank 0.  One deviation: the reference adds `float(loss)` to
its running loss every step, which waits for the device once per step; this loop keeps the step losses on the device
and averages them at each evaluation, as the engine path does.  The default, `engine`, is gist_amd.ist.train.
"""
import argparse
import random

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F


def add_ist_args(parser):
    """The flags the reference's IST scripts share (cluster_gcn_ist_distrib.py:520-559,
    cluster_gcn_ist_distrib_gat.py:538-577)."""
    from gist_amd.dgl_compat.data import register_data_args
    register_data_args(parser)
    parser.add_argument("--iter_per_site", type=int, default=5)
    parser.add_argument("--num_subnet", type=int, default=2, help="number of sub networks")
    parser.add_argument("--dropout", type=float, default=0.5, help="dropout probability")
    parser.add_argument("--lr", type=float, default=0.01, help="learning rate")
    parser.add_argument("--n-epochs", type=int, default=20, help="number of training epochs")
    parser.add_argument("--n-hidden", type=int, default=16, help="number of hidden gcn units")
    parser.add_argument("--n-layers", type=int, default=1, help="number of hidden gcn layers")
    parser.add_argument("--weight-decay", type=float, default=5e-4, help="Weight for L2 loss")
    parser.add_argument("--use_layernorm", type=bool, default=False)
    parser.add_argument('--dist-backend', type=str, default='nccl')
    parser.add_argument('--dist-url', type=str, default='tcp://127.0.0.1:9971')
    parser.add_argument('--rank', type=int, default=0)
    parser.add_argument('--cuda-id', type=int, default=0)
    parser.add_argument("--batch-size", type=int, default=20, help="batch size")
    parser.add_argument("--psize", type=int, default=1500, help="partition number")
    parser.add_argument("--test-batch-size", type=int, default=1000)
    parser.add_argument("--rnd-seed", type=int, default=3)
    parser.add_argument("--use-pp", action='store_true')
    parser.add_argument("--normalize", action='store_true')
    parser.add_argument("--save_results", action='store_true')
    return parser


def build_parser():
    parser = add_ist_args(argparse.ArgumentParser(description='GCN'))
    parser.add_argument("--fig-dir", type=str, default='../report/example_pic/')
    parser.add_argument("--fig-name", type=str, default='name')
    parser.add_argument("--use-f1", action='store_true')
    # (not a flag of the reference) module: the reference's loop on ist_model.sub_model / base_model (main_module_path);
    # engine: gist_amd.ist.train, one gist_sage_step per iteration
    parser.add_argument("--host-path", choices=['engine', 'module'], default='engine')
    return parser


def save_results(args, res, log=print):
    """:455-473 -- with --save_results the reference writes `{fig_name}_result.pckl` (total_time,
    trn_losses, val_accs, test_accs) under --fig-dir, which its sweep drivers read back
    (script/reddit/run_ist_sweep_reddit.py), INSTEAD of printing the five result lines.  The
    validation-accuracy PNG of :457-461 is not produced (matplotlib reporting is out of scope)."""
    import os
    import pickle
    os.makedirs(args.fig_dir, exist_ok=True)
    results = {'total_time': res['total_time'], 'trn_losses': res['trn_losses'],
               'val_accs': res['val_accs'], 'test_accs': res['test_accs']}
    path = os.path.join(args.fig_dir, args.fig_name + '_result.pckl')
    with open(path, 'wb') as f:
        pickle.dump(results, f)
    return path


def setup(args, dataset=None, log=print):
    """:565-591 -- seeds (the same on every rank), this rank's device, the process group of num_subnet ranks, the
    dataset (`dataset` given: used instead of load_data) and --normalize.  Returns (device, data, g, in_feats,
    n_classes, train_nid, par_li, psize); `g` stays on the host."""
    from gist_amd.dgl_compat.data import load_data
    log('Setting seeds', flush=True)
    torch.manual_seed(args.rnd_seed)                        # :570-572, same seed on every rank
    np.random.seed(args.rnd_seed)
    random.seed(args.rnd_seed)
    assert args.cuda_id < torch.cuda.device_count()
    device = torch.device(f'cuda:{args.cuda_id}')
    torch.cuda.set_device(device)
    log(f'{args.rank} initializing process', flush=True)
    dist.init_process_group(backend=args.dist_backend, init_method=args.dist_url,
                            rank=args.rank, world_size=args.num_subnet)
    data = dataset if dataset is not None else load_data(args)
    g = data.g
    if args.normalize:                 # StandardScaler fit on the train rows, on the device
        from gist_amd import hip
        feats = g.ndata['feat'].to(device).contiguous()
        fit = torch.nonzero(g.ndata['train_mask'].to(device)).flatten().to(torch.int32)
        hip.standard_scale_(feats, fit)
        g.ndata['feat'] = feats
    in_feats, n_classes = g.ndata['feat'].shape[1], data.num_classes
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    par_li = getattr(data, 'par_li', None)
    psize = len(par_li) if par_li is not None else args.psize
    return device, data, g, in_feats, n_classes, train_nid, par_li, psize


def add_family_args(parser, family):
    """--exp_name and (not flags of the reference) --host-path and --eval-path of a family's GIST script: host_path and
    eval_path of its gist_amd.ist loop, the choices those the wrapper class `family` states."""
    parser.add_argument("--exp_name", type=str, default='distributed_gnn_ist')
    parser.add_argument("--host-path", choices=['module', family.STEP_PATH] + (['phases'] if family.PHASES else []),
                        default='module')
    if len(family.EVAL_PATHS) > 1:
        parser.add_argument("--eval-path", choices=list(family.EVAL_PATHS), default='layers')
    return parser


def report_family(args, res, log, lines):
    """With --save_results the pickle {total_time, trn_losses, val_accs, test_accs} goes to
    ./results/{exp_name}_result.pckl (returns its path); otherwise lines(res, log=log) prints the result lines."""
    if args.save_results:
        import os
        import pickle
        os.makedirs('./results', exist_ok=True)
        path = os.path.join('./results', args.exp_name + '_result.pckl')
        with open(path, 'wb') as f:
            pickle.dump({'total_time': res['total_time'], 'trn_losses': res['trn_losses'],
                         'val_accs': res['val_accs'], 'test_accs': res['test_accs']}, f)
        return path
    lines(res, log=log)
    return None


def main_family(args, dataset, log, setup, wrapper, train, report, comm=None):
    """The body of a family's GIST script after its own refusals: its set-up, the iterator (get_data: one shuffle; the
    one-call path's describes its batches), the family's wrapper, the initial dispatch, its gist_amd.ist loop `train`,
    rank 0's report, the end of the group.

    setup, wrapper, train and report are handed in, and the sampler's classes are looked up when this runs, because each
    family script resolves them in its own namespace or on gist_amd.ist at call time: a test that stands in for one of
    them there (tests/test_baseline_gcn_ist.py does, for all four and for EngineClusterIter) must be what runs here.
    use_pp reaches the iterator only when it is set (its default is off): a family that refuses --use-pp never names it."""
    import gist_amd.sampler as sampler
    assert (args.n_hidden % args.num_subnet) == 0
    host_path = getattr(args, 'host_path', 'module')
    device, data, g, in_feats, n_classes, train_nid, par_li, psize = setup(args, dataset, log)
    iter_cls = sampler.ClusterIter if host_path in ('module', 'phases') else sampler.EngineClusterIter
    cluster_iterator = iter_cls(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li, device=device,
                                **(dict(use_pp=True) if args.use_pp else {}))
    g = g.to(device)
    ist_model = wrapper(args, g, in_feats, n_classes, device, comm=comm, seed=args.rnd_seed)
    log(f'{args.rank}: start initial dispatch', flush=True)
    ist_model.ini_sync_dispatch_model()
    log(f'{args.rank}: finish initial dispatch', flush=True)
    paths = dict(host_path=host_path)
    if hasattr(args, 'eval_path'):                   # (a family with one evaluator has no --eval-path)
        paths['eval_path'] = args.eval_path
    res = train(ist_model, args, g, cluster_iterator, g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask'],
                log=log, **paths)
    if args.rank == 0:
        path = report(args, res, log=log)
        if path is not None:
            res['results_path'] = path
    dist.destroy_process_group()
    res['model'] = ist_model
    return res


def main(args=None, dataset=None, log=print, ultra_wide=False):
    from gist_amd import ist
    from gist_amd.modules import GCN
    from gist_amd.sampler import EngineClusterIter
    from gist_amd.trainer import FullGraphEvaluator
    if args is None:
        args = build_parser().parse_args()
    assert (args.n_hidden % args.num_subnet) == 0
    if args.use_pp:
        raise NotImplementedError(
            'gist_amd: --use-pp cannot work with GCN / ISTSAGELayer in the reference either (the '
            'feature width doubles after in_feats was read, SURVEY.md appendix C.8); the layer-0 '
            'pre-aggregation is offered as ClusterIter(..., use_pp=True) + GraphSAGE-style layers')
    if args.use_f1:
        log('note: --use-f1 reports micro-F1, which equals argmax accuracy for single-label '
            'classification (cluster_gcn/utils.py:47-67)', flush=True)
    device, data, g, in_feats, n_classes, train_nid, par_li, psize = setup(args, dataset, log)
    if getattr(args, 'host_path', 'engine') == 'module':
        if ultra_wide:
            raise SystemExit('gist_amd: --host-path module is not offered for cluster_gcn_ist_ultra_wide (its '
                             'evaluation needs the bounded row block of the engine path); use --host-path engine')
        res = main_module_path(args, g, device, in_feats, n_classes, train_nid, par_li, psize, log)
        dist.destroy_process_group()
        return res
    it = EngineClusterIter(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li,
                           device=device)                    # :507-509 (one shuffle)
    base_init = None
    if args.rank == 0:                                       # :78-85 rank 0 builds the base model
        base = GCN(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout,
                   args.use_layernorm, False, False, 1, True)
        base_init = [(l.linear.weight.detach(), l.linear.bias.detach()) for l in base.layers]
    model = ist.DistributedGNNWrapper(args, g, in_feats, n_classes, device, base_init=base_init,
                                      n_max=it.n_max, seed=args.rnd_seed)
    log(f'{args.rank}: start initial dispatch', flush=True)
    model.ini_sync_dispatch_model()                          # :595
    log(f'{args.rank}: finish initial dispatch', flush=True)
    it.bind(model.engine)
    evaluator = None
    if args.rank == 0:
        # ultra-wide (cluster_gcn_ist_ultra_wide.py:500-504 evaluates on the CPU because [N, 2H]
        # does not fit its GPU): the evaluator works block of rows by block of rows in HBM
        evaluator = FullGraphEvaluator(g, model.base_dims, args.use_layernorm, model.base, device,
                                       block_bytes=(1 << 30) if ultra_wide else (4 << 30))
    res = ist.train(model, args, it, evaluator=evaluator, log=log)
    if args.rank == 0:
        if args.save_results:
            log('results written to %s' % save_results(args, res, log=log), flush=True)
        else:
            ist.print_results(res, log=log)                  # :475-479
    dist.destroy_process_group()
    res['model'] = model
    return res


def main_module_path(args, g, device, in_feats, n_classes, train_nid, par_li, psize, log):
    """cluster_gcn_ist_distrib.py:370-479 + :593-597 on the drop-in classes.  The step losses stay on the device (the
    reference's per-step `float(loss)`, :416, would wait for the device once per step); each evaluation averages them.
    Returns what gist_amd.ist.train returns (total_time, losses, events, accuracies) plus the wrapper as 'model'."""
    import time
    from gist_amd import ist
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    from gist_amd.utils import evaluate
    cluster_iterator = ClusterIter(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li,
                                   device=device)                                    # :507-509 (one shuffle)
    ist_model = ist.DistributedGNNWrapper(args, g, in_feats, n_classes, device, seed=args.rnd_seed)    # :593
    log(f'{args.rank}: start initial dispatch', flush=True)
    ist_model.ini_sync_dispatch_model()                                              # :595
    log(f'{args.rank}: finish initial dispatch', flush=True)
    labels, val_mask, test_mask = g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask']
    multi = dist.get_world_size() > 1
    method = 'f1' if args.use_f1 else 'acc'
    test_accs, val_accs, trn_losses, losses, events = [], [], [], [], []
    loss_fcn = CrossEntropyLoss()                                                    # :384
    local_epochs = args.n_epochs // args.num_subnet
    running, total_iter, total_time = [], 0, 0.
    torch.cuda.synchronize(device)
    start_time = time.time()
    for e in range(local_epochs):
        log(f'{args.rank}: running epoch {e} / {local_epochs}', flush=True)
        lr = args.lr
        run_eval = True
        for j, cluster in enumerate(cluster_iterator):
            if total_iter % args.iter_per_site == 0:                                 # :400-407
                if e > 0:
                    if multi:
                        dist.barrier()
                    ist_model.dispatch_model()
                    events.append('dispatch')
                ist_model.sub_model.train()
                optimizer = Adam(ist_model.sub_model.parameters(), lr=lr, weight_decay=args.weight_decay)
            optimizer.zero_grad()                                                    # :408-417
            cluster = cluster.to(device)
            pred = ist_model.sub_model(cluster)
            batch_labels = cluster.ndata['label']
            batch_train_mask = cluster.ndata['train_mask']
            loss = loss_fcn(pred[batch_train_mask], batch_labels[batch_train_mask])
            loss.backward()
            running.append(loss.detach())
            optimizer.step()
            events.append('step')
            total_iter += 1
            last = (j == len(cluster_iterator) - 1) and (e == local_epochs - 1)
            if total_iter % args.iter_per_site == 0 or last:                         # :422-450
                if multi:
                    dist.barrier()
                ist_model.sync_model()
                events.append('sync')
                if run_eval or last:
                    torch.cuda.synchronize(device)
                    total_time += time.time() - start_time
                    run_eval = False
                    events.append('eval')
                    if args.rank == 0:
                        val_accs.append(evaluate(ist_model.base_model, g, labels, val_mask, method))
                        test_accs.append(evaluate(ist_model.base_model, g, labels, test_mask, method))
                        trn_losses.append(float(torch.stack(running).mean().item()) if running else 0.0)
                    losses.extend(running)
                    running = []
                    torch.cuda.synchronize(device)
                    start_time = time.time()
    losses.extend(running)
    if multi:
        dist.barrier()
    res = dict(total_time=total_time, losses=[losses], events=events, val_accs=val_accs, test_accs=test_accs,
               trn_losses=trn_losses, model=ist_model)
    if args.rank == 0:
        if args.save_results:
            log('results written to %s' % save_results(args, res, log=log), flush=True)
        else:
            ist.print_results(res, log=log)                                          # :475-479
    return res


if __name__ == '__main__':
    import os
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    main()
