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

from gist_amd import ist
# (dist: the process group setup() opens and main_family ends)
from gist_amd.scripts.cluster_gcn_ist_distrib import add_family_args, add_ist_args, dist, main_family, report_family, setup

FAMILY = ist.DistributedGraphSAGEWrapper        # its facts are the choices of --host-path and --eval-path


def build_parser():
    return add_family_args(add_ist_args(argparse.ArgumentParser(description='GCN')), FAMILY)


def report(args, res, log=print):
    """With --save_results the pickle {total_time, trn_losses, val_accs, test_accs} goes to
    ./results/{exp_name}_result.pckl (returns its path); otherwise the five result lines (:475-479)."""
    return report_family(args, res, log, ist.print_results)


def main(args=None, dataset=None, log=print, comm=None):
    """comm: the wrapper's collectives (None: gist_amd.ist.TorchDistComm over the process group set up here)."""
    if args is None:
        args = build_parser().parse_args()
    if args.cuda_id < 0:
        raise SystemExit('gist_amd: the GraphSAGE family runs on a GPU (--cuda-id >= 0)')
    log('note: --use_layernorm %s: the GraphSAGE family\'s LayerNorm is always on (every layer but the output layer)'
        % args.use_layernorm, flush=True)
    # (the wrapper and the loop as gist_amd.ist has them now: a stand-in there is what runs)
    return main_family(args, dataset, log, setup, ist.DistributedGraphSAGEWrapper, ist.train_graphsage, report, comm=comm)


if __name__ == '__main__':
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    main()
