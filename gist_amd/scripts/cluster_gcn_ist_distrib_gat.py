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

from gist_amd import ist
# (dist: the process group setup() opens and main_family ends)
from gist_amd.scripts.cluster_gcn_ist_distrib import add_family_args, add_ist_args, dist, main_family, report_family, setup

FAMILY = ist.DistributedGATWrapper        # its facts are the choices of --host-path and --eval-path


def build_parser():
    parser = add_ist_args(argparse.ArgumentParser(description='GCN'))
    parser.add_argument('--n-heads', type=int, default=4)
    # (not a flag of the reference) cat: the hidden layers concatenate their heads (its comment, modules.py:87-89)
    parser.add_argument('--head-merge', choices=['mean', 'cat'], default='mean')
    # --host-path module: the reference's loop on ist_model.sub_model / base_model; engine: one gist_gat_step per
    # iteration; phases: the module loop with sub_model bound to the iterator, three gist_gat_step_phase calls per
    # iteration.  --eval-path blocked: rank 0's evaluate(base_model, g, ...) runs gist_amd.gat_eval's
    # GATFullGraphEvaluator instead of the model's own forward (gist_amd.ist.train_gat)
    return add_family_args(parser, FAMILY)


def _four_lines(res, log=print):
    """:494-499 -- exactly four lines in the reference's order, which its sweep reads by position."""
    log(f"Training Time: {res['total_time']:.4f}")
    log(f"Last Test: {res['test_accs'][-1]:.4f}")
    log(f"Best Test: {max(res['test_accs']):.4f}")
    log(f"Best Val: {max(res['val_accs']):.4f}")


def report(args, res, log=print):
    """:481-499 -- the results pickle with --save_results (returns its path), otherwise the four result lines."""
    return report_family(args, res, log, _four_lines)


def main(args=None, dataset=None, log=print):
    if args is None:
        args = build_parser().parse_args()
    host_path = getattr(args, 'host_path', 'module')
    if host_path in ('engine', 'phases') and (args.use_pp or args.cuda_id < 0):
        raise SystemExit('gist_amd: --host-path %s is the fused GAT step: it runs on a GPU (--cuda-id >= 0) and '
                         'extracts its batches from the plain features (no --use-pp); use --host-path module'
                         % host_path)
    if args.use_pp:
        raise NotImplementedError(
            'gist_amd: --use-pp cannot work with the GAT in the reference either (the feature width doubles after '
            'in_feats was read)')
    # (the wrapper and the loop as gist_amd.ist has them now: a stand-in there is what runs)
    return main_family(args, dataset, log, setup, ist.DistributedGATWrapper, ist.train_gat, report)


if __name__ == '__main__':
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    main()
