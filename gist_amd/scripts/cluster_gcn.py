#!/usr/bin/env python3
"""Single-GPU Cluster-GCN training -- CLI and output contract of the reference's
cluster_gcn/cluster_gcn.py (flags :145-180, five result lines :132-136), running on the
gist_amd HIP path.

    python -m gist_amd.scripts.cluster_gcn --dataset reddit-synth --lr 0.01 --n-epochs 80 \\
        --batch-size 20 --n-hidden 256 --n-layers 4 --dropout 0.2 --use-layernorm --rnd-seed 0

Datasets are the seeded synthetic stand-ins of gist_amd.datasets (no real data offline);
their block structure supplies the partition list in place of METIS.
"""
import argparse
import random

import numpy as np
import torch
import torch.nn.functional as F


def build_parser():
    parser = argparse.ArgumentParser(description='GCN')
    from gist_amd.dgl_compat.data import register_data_args
    register_data_args(parser)
    parser.add_argument("--dropout", type=float, default=0.2, help="dropout probability")
    parser.add_argument("--gpu", type=int, default=0, help="gpu")
    parser.add_argument("--lr", type=float, default=3e-2, help="learning rate")
    parser.add_argument("--n-epochs", type=int, default=40, help="number of training epochs")
    parser.add_argument("--batch-size", type=int, default=20, help="batch size")
    parser.add_argument("--psize", type=int, default=1500, help="partition number")
    parser.add_argument("--test-batch-size", type=int, default=1000, help="test batch size")
    parser.add_argument("--n-hidden", type=int, default=128, help="number of hidden gcn units")
    parser.add_argument("--n-layers", type=int, default=1, help="number of hidden gcn layers")
    parser.add_argument("--rnd-seed", type=int, default=3)
    parser.add_argument("--use-pp", action='store_true', help="whether to use precomputation")
    parser.add_argument("--normalize", action='store_true', help="whether to use normalized feature")
    parser.add_argument("--weight-decay", type=float, default=0, help="Weight for L2 loss")
    parser.add_argument("--model-type", type=str, default='sage', help="sage, gat, graphsage or baseline")
    parser.add_argument("--n-heads", type=int, default=4, help="attention heads of the GAT layers")
    # (not a flag of the reference) cat: the hidden GAT layers concatenate their heads (its comment, modules.py:87-89)
    parser.add_argument("--head-merge", choices=['mean', 'cat'], default='mean',
                        help="how a GAT layer combines its heads")
    parser.add_argument("--fig-dir", type=str, default='../report/example_pic/')
    parser.add_argument("--fig-name", type=str, default='name')
    parser.add_argument("--use-layernorm", action='store_true')
    parser.add_argument("--use-f1", action='store_true')
    parser.add_argument("--eval-cpu", action='store_true')
    # (not a flag of the reference) module: the reference's own loop body, statement for statement, on gist_amd.modules.GCN /
    # nn.CrossEntropyLoss / optim.Adam / sampler.ClusterIter (gist_amd/module_engine.py); engine: one gist_sage_step (sage) or
    # gist_gat_step (gat) per iteration; phases (gat): the module loop with the model bound to its iterator
    # (module_engine.bind_gat) -- the engine's launches as three gist_gat_step_phase calls per iteration; step (graphsage):
    # one gist_graphsage_step per iteration (gist_amd/graphsage_engine.py); step (baseline): one gist_baseline_gcn_step per
    # iteration (gist_amd/baseline_gcn_engine.py); engine and module keep those families' module loop
    parser.add_argument("--host-path", choices=['engine', 'module', 'phases', 'step'], default='engine')
    # (not a flag of the reference; --model-type gat and graphsage) how evaluate() runs the full-graph forward: layers = the model's own
    # forward, layer by layer on the training kernels; blocked = gist_amd.gat_eval.GATFullGraphEvaluator (preallocated
    # buffers, two-pass softmax, the graph's node blocks as dense products on the matrix cores); rows (--model-type
    # graphsage) = gist_amd.graphsage_eval.GraphSAGEFullGraphEvaluator (preallocated buffers, row block by row block, the
    # node blocks on the matrix cores, layer 0's aggregation kept, a tail kernel that stores its result alone)
    parser.add_argument("--eval-path", choices=['layers', 'blocked', 'rows'], default='layers')
    return parser


def attach_eval_path(args, model, arena=None):
    """--eval-path blocked: route evaluate(model, g, ...) through a GATFullGraphEvaluator; --eval-path rows: through a
    GraphSAGEFullGraphEvaluator."""
    if getattr(args, 'eval_path', 'layers') == 'blocked':
        from gist_amd.gat_eval import GATFullGraphEvaluator
        GATFullGraphEvaluator.attach(model, arena=arena)
    elif getattr(args, 'eval_path', 'layers') == 'rows':
        from gist_amd.graphsage_eval import GraphSAGEFullGraphEvaluator
        GraphSAGEFullGraphEvaluator.attach(model, arena=arena)


def load_graph(args, dataset, log):
    """the dataset's graph, the device, and the sizes every path of main needs (cluster_gcn.py:24-43)"""
    from gist_amd.dgl_compat.data import load_data
    data = dataset if dataset is not None else load_data(args)
    g = data.g
    device = torch.device('cuda', args.gpu)
    torch.cuda.set_device(device)
    if args.normalize:                 # StandardScaler fit on the train rows, on the device
        from gist_amd import hip
        feats = g.ndata['feat'].to(device).contiguous()
        fit = torch.nonzero(g.ndata['train_mask'].to(device)).flatten().to(torch.int32)
        hip.standard_scale_(feats, fit)
        g.ndata['feat'] = feats
    in_feats = g.ndata['feat'].shape[1]
    n_classes = data.num_classes
    par_li = getattr(data, 'par_li', None)
    psize = len(par_li) if par_li is not None else args.psize
    log('labels shape:', g.ndata['label'].shape)
    log("features shape, ", g.ndata['feat'].shape)
    return data, g, device, in_feats, n_classes, par_li, psize


def main(args, dataset=None, log=print):
    from gist_amd.modules import GCN
    from gist_amd.trainer import ClusterGCNTrainer
    torch.manual_seed(args.rnd_seed)                       # cluster_gcn.py:20-22
    np.random.seed(args.rnd_seed)
    random.seed(args.rnd_seed)
    if args.gpu < 0 or args.eval_cpu:
        raise SystemExit('gist_amd runs on the GPU only (no CPU fallback): --gpu >= 0, no --eval-cpu')
    if args.model_type == 'baseline':
        return main_baseline(args, dataset, log)
    if args.model_type not in ('sage', 'gat', 'graphsage'):
        raise NotImplementedError(f'{args.model_type} is not a supported model type')
    if getattr(args, 'eval_path', 'layers') == 'rows' and args.model_type != 'graphsage':
        raise SystemExit('gist_amd: --eval-path rows is the GraphSAGE family\'s evaluator (--model-type graphsage); the SAGE '
                         'engine path already evaluates with trainer.FullGraphEvaluator, the GAT has --eval-path blocked')
    data, g, device, in_feats, n_classes, par_li, psize = load_graph(args, dataset, log)
    # construction order as in the reference: ClusterIter (one shuffle) before the model
    model_holder = {}

    def make_model():
        m = GCN(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout,
                args.use_layernorm, False, False, 1, True)          # :66-69
        model_holder['m'] = m
        return m
    host_path = getattr(args, 'host_path', 'engine')
    if getattr(args, 'eval_path', 'layers') == 'blocked' and args.model_type != 'gat':
        raise SystemExit('gist_amd: --eval-path blocked is the GAT evaluator (--model-type gat); the SAGE engine path '
                         'already evaluates with trainer.FullGraphEvaluator')
    if host_path == 'phases' and args.model_type != 'gat':
        raise SystemExit('gist_amd: --host-path phases binds a GAT to its iterator (--model-type gat); the SAGE module '
                         'path already runs on the phase calls of the fused step: use --host-path module')
    if host_path == 'step' and args.model_type != 'graphsage':
        raise SystemExit('gist_amd: --host-path step is the one-call step of the GraphSAGE and BaselineGCN families '
                         '(--model-type graphsage, baseline); the other families run theirs under --host-path engine')
    if args.model_type == 'graphsage' and host_path == 'step':
        return main_graphsage_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log)
    if args.model_type == 'graphsage':
        # modules.GraphSAGE (the model --use-pp was written for): its fused step is opt-in (--host-path step); every other
        # host path keeps the reference's loop on its layers
        log('--model-type graphsage has no fused step: --host-path %s runs the module loop, layer by layer' % host_path)
        return main_module_path(args, data, g, device, in_feats, n_classes, par_li, psize, log)
    if args.model_type == 'gat' and host_path == 'engine' and not args.use_pp:
        return main_gat_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log)
    if args.model_type == 'gat' or host_path == 'module':
        # (--host-path phases: the same loop, the GAT bound to the iterator first)
        # (--use-pp changes the train graph's features under the iterator: the GAT then keeps the reference's loop)
        return main_module_path(args, data, g, device, in_feats, n_classes, par_li, psize, log)
    trainer = ClusterGCNTrainer(args.dataset, g, par_li, psize, args.batch_size, args.n_hidden,
                                args.n_layers, n_classes, args.dropout, args.use_layernorm,
                                args.lr, args.weight_decay, device, seed=args.rnd_seed)
    trainer.engine.arena.adopt_module(make_model())        # same-seed init as the reference
    val_accs, test_accs = [], []
    for epoch in range(args.n_epochs):                     # :89-127
        log(f'Running epoch {epoch} / {args.n_epochs}', flush=True)
        trainer.timed_epoch()
        val_accs.append(trainer.evaluate('val_mask'))
        test_accs.append(trainer.evaluate('test_mask'))
        log(f'Val acc {val_accs[-1]}', flush=True)
    log(f'Training Time: {trainer.total_time:.4f}', flush=True)    # :132-136
    log(f'Last Val: {val_accs[-1]:.4f}', flush=True)
    log(f'Best Val: {max(val_accs):.4f}', flush=True)
    log(f'Last Test: {test_accs[-1]:.4f}', flush=True)
    log(f'Best Test: {max(test_accs):.4f}', flush=True)
    return dict(total_time=trainer.total_time, val_accs=val_accs, test_accs=test_accs,
                model=model_holder['m'])


def main_baseline(args, dataset, log):
    """--model-type baseline: modules.BaselineGCN (cluster_gcn/modules.py:316-349, the plain GCN of GraphConv layers) in
    the reference's loop body; its fused step is opt-in (--host-path step, main_baseline_engine).  The family has no
    precomputation and no evaluator of its own: the model's own full-graph forward evaluates, its tail in place."""
    if args.use_pp:
        raise SystemExit('gist_amd: --use-pp is the GraphSAGE layer\'s precomputation (--model-type graphsage); '
                         '--model-type baseline aggregates in every layer')
    if getattr(args, 'eval_path', 'layers') != 'layers':
        raise SystemExit('gist_amd: --eval-path %s is another family\'s evaluator; --model-type baseline evaluates with '
                         'its own full-graph forward (--eval-path layers)' % args.eval_path)
    host_path = getattr(args, 'host_path', 'engine')
    if host_path == 'step':
        data, g, device, in_feats, n_classes, par_li, psize = load_graph(args, dataset, log)
        return main_baseline_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log)
    if host_path != 'module':
        log('--model-type baseline has no fused step under --host-path %s (its step is --host-path step): the module loop '
            'runs, layer by layer' % host_path)
    data, g, device, in_feats, n_classes, par_li, psize = load_graph(args, dataset, log)
    return main_module_path(args, data, g, device, in_feats, n_classes, par_li, psize, log)


def engine_epochs(args, it, engine, model, g, device, log):
    """The epochs of the one-call paths (main_baseline_engine, main_gat_engine, main_graphsage_engine): one train_step per
    batch of `it`, timed per epoch between two synchronises; `model`, whose parameters are the engine's arena, evaluated
    on the device graph `g` after each; the five result lines.  -> (total_time, val_accs, test_accs)."""
    import time
    from gist_amd.utils import evaluate
    labels, val_mask, test_mask = g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask']
    total_time, val_accs, test_accs = 0., [], []
    for epoch in range(args.n_epochs):                     # cluster_gcn.py:89-127
        log(f'Running epoch {epoch} / {args.n_epochs}', flush=True)
        torch.cuda.synchronize(device)
        start_time = time.time()
        for batch in it:
            engine.train_step(batch, args.lr, args.weight_decay)
        torch.cuda.synchronize(device)
        total_time += time.time() - start_time
        engine.check_extract()                             # (outside the timed interval)
        val_accs.append(evaluate(model, g, labels, val_mask, 'f1' if args.use_f1 else 'acc'))
        test_accs.append(evaluate(model, g, labels, test_mask, 'f1' if args.use_f1 else 'acc'))
        log(f'Val acc {val_accs[-1]}', flush=True)
    log(f'Training Time: {total_time:.4f}', flush=True)    # :132-136
    log(f'Last Val: {val_accs[-1]:.4f}', flush=True)
    log(f'Best Val: {max(val_accs):.4f}', flush=True)
    log(f'Last Test: {test_accs[-1]:.4f}', flush=True)
    log(f'Best Test: {max(test_accs):.4f}', flush=True)
    return total_time, val_accs, test_accs


def main_baseline_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log):
    """--model-type baseline --host-path step: one gist_baseline_gcn_step per iteration (gist_amd/baseline_gcn_engine.py),
    fed by EngineClusterIter.  Same construction order, RNG draws for the weights and batch order as main_module_path;
    the dropout masks come from autograd.gcn_tail's generator, seed and counter scheme, counted by the engine from 0
    instead of by the process-wide counter."""
    from gist_amd.arena import baseline_gcn_dims
    from gist_amd.baseline_gcn_engine import BaselineGCNEngine
    from gist_amd.modules import BaselineGCN
    from gist_amd.sampler import EngineClusterIter
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li, device=device)
    g = g.to(device)
    model = BaselineGCN(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout, args.use_layernorm)
    model.cuda()
    model.set_dropout_seed(args.rnd_seed)
    engine = BaselineGCNEngine(baseline_gcn_dims(in_feats, args.n_hidden, n_classes, args.n_layers), args.use_layernorm,
                               args.dropout, it.n_max, device, seed=args.rnd_seed)
    engine.bind(model)                                     # the model's parameters are the arena's views from here on
    it.bind(engine)
    engine.prefetch = True                                 # (the loop only reads the loss of a step)
    total_time, val_accs, test_accs = engine_epochs(args, it, engine, model, g, device, log)
    return dict(total_time=total_time, val_accs=val_accs, test_accs=test_accs, model=model, engine=engine)


def main_gat_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log):
    """--model-type gat on the fused step: one gist_gat_step per iteration (gist_amd/gat_engine.py), fed by
    EngineClusterIter.  Same construction order, RNG draws, batch order and arithmetic as main_module_path: same-seed
    weights are bit-identical whatever the host path."""
    from gist_amd.gat_engine import GATEngine
    from gist_amd.ist import gat_dims, gat_params
    from gist_amd.modules import GAT
    from gist_amd.sampler import EngineClusterIter
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter(args.dataset, g, psize, args.batch_size, train_nid, par_li=par_li, device=device)
    g = g.to(device)
    merge = getattr(args, 'head_merge', 'mean')
    model = GAT(args.n_layers, in_feats, args.n_hidden, n_classes, args.n_heads,   # cluster_gcn_ist_distrib_gat.py:77-79
                merge=merge)
    engine = GATEngine(gat_dims(in_feats, args.n_hidden, n_classes, args.n_layers, args.n_heads, merge), it.n_max,
                       device)
    engine.arena.load(gat_params(model))
    engine.bind(model)                                     # the model's parameters are the arena's views from here on
    it.bind(engine)
    engine.prefetch = True                                 # (the loop only reads the loss of a step)
    attach_eval_path(args, model, engine.arena)
    total_time, val_accs, test_accs = engine_epochs(args, it, engine, model, g, device, log)
    return dict(total_time=total_time, val_accs=val_accs, test_accs=test_accs, model=model)


def main_graphsage_engine(args, data, g, device, in_feats, n_classes, par_li, psize, log):
    """--model-type graphsage --host-path step: one gist_graphsage_step per iteration (gist_amd/graphsage_engine.py), fed
    by EngineClusterIter (with --use-pp: its [X | A^X] features).  Same construction order, RNG draws for the weights and
    batch order as main_module_path; the dropout masks come from the step's counter-based generator, not torch's."""
    from gist_amd.arena import graphsage_dims
    from gist_amd.graphsage_engine import GraphSAGEEngine
    from gist_amd.modules import GraphSAGE
    from gist_amd.sampler import EngineClusterIter
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    it = EngineClusterIter(args.dataset, g, psize, args.batch_size, train_nid, use_pp=args.use_pp, par_li=par_li,
                           device=device)
    g = g.to(device)
    model = GraphSAGE(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout, args.use_pp)
    model.cuda()
    engine = GraphSAGEEngine(graphsage_dims(in_feats, args.n_hidden, n_classes, args.n_layers), args.dropout, it.n_max,
                             device, seed=args.rnd_seed, use_pp=args.use_pp)
    engine.bind(model)                                     # the model's parameters are the arena's views from here on
    it.bind(engine)
    engine.prefetch = True                                 # (the loop only reads the loss of a step)
    attach_eval_path(args, model, engine.arena)
    total_time, val_accs, test_accs = engine_epochs(args, it, engine, model, g, device, log)
    return dict(total_time=total_time, val_accs=val_accs, test_accs=test_accs, model=model, engine=engine)


def main_module_path(args, data, g, device, in_feats, n_classes, par_li, psize, log):
    """cluster_gcn/cluster_gcn.py:24-136 on the drop-in classes: ClusterIter, GCN (or GAT, GraphSAGE, BaselineGCN),
    CrossEntropyLoss, Adam, evaluate."""
    import time
    from gist_amd.modules import GAT, GCN, BaselineGCN, GraphSAGE
    from gist_amd.nn import CrossEntropyLoss
    from gist_amd.optim import Adam
    from gist_amd.sampler import ClusterIter
    from gist_amd.utils import evaluate
    train_nid = np.nonzero(g.ndata['train_mask'].numpy())[0].astype(np.int64)
    cluster_iterator = ClusterIter(args.dataset, g, psize, args.batch_size, train_nid, use_pp=args.use_pp,
                                   par_li=par_li, device=device)                                      # :44-46
    g = g.to(device)
    labels, val_mask, test_mask = g.ndata['label'], g.ndata['val_mask'], g.ndata['test_mask']
    if args.model_type == 'gat':
        model = GAT(args.n_layers, in_feats, args.n_hidden, n_classes, args.n_heads,   # cluster_gcn_ist_distrib_gat.py:77-79
                    merge=getattr(args, 'head_merge', 'mean'))
        model.cuda()
    elif args.model_type == 'graphsage':
        model = GraphSAGE(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout, args.use_pp)
        model.cuda()
    elif args.model_type == 'baseline':
        model = BaselineGCN(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout, args.use_layernorm)
        model.cuda()
        model.set_dropout_seed(args.rnd_seed)
    else:
        model = GCN(in_feats, args.n_hidden, n_classes, args.n_layers, F.relu, args.dropout,
                    args.use_layernorm, False, False, 1, True)                                         # :66-69
        model.cuda()
        model.set_dropout_seed(args.rnd_seed)
    if args.model_type == 'gat' and getattr(args, 'host_path', 'engine') == 'phases':
        from gist_amd.module_engine import bind_gat
        bind_gat(model, cluster_iterator)            # model(cluster), loss.backward(), optimizer.step(): the fused step's phases
    if args.model_type in ('gat', 'graphsage'):
        attach_eval_path(args, model)
    loss_f = CrossEntropyLoss()                                                                        # :76
    optimizer = Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)                   # :77-80
    total_time, val_accs, test_accs = 0., [], []
    for epoch in range(args.n_epochs):                                                                 # :89-127
        log(f'Running epoch {epoch} / {args.n_epochs}', flush=True)
        torch.cuda.synchronize(device)
        start_time = time.time()
        for j, cluster in enumerate(cluster_iterator):
            cluster = cluster.to(torch.cuda.current_device())
            model.train()
            pred = model(cluster)
            batch_labels = cluster.ndata['label']
            batch_train_mask = cluster.ndata['train_mask']
            loss = loss_f(pred[batch_train_mask], batch_labels[batch_train_mask])
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        torch.cuda.synchronize(device)
        total_time += time.time() - start_time
        val_accs.append(evaluate(model, g, labels, val_mask, 'f1' if args.use_f1 else 'acc'))
        test_accs.append(evaluate(model, g, labels, test_mask, 'f1' if args.use_f1 else 'acc'))
        log(f'Val acc {val_accs[-1]}', flush=True)
    log(f'Training Time: {total_time:.4f}', flush=True)                                                # :132-136
    log(f'Last Val: {val_accs[-1]:.4f}', flush=True)
    log(f'Best Val: {max(val_accs):.4f}', flush=True)
    log(f'Last Test: {test_accs[-1]:.4f}', flush=True)
    log(f'Best Test: {max(test_accs):.4f}', flush=True)
    return dict(total_time=total_time, val_accs=val_accs, test_accs=test_accs, model=model)


if __name__ == '__main__':
    import os
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    a = build_parser().parse_args()
    print(a)
    main(a)
