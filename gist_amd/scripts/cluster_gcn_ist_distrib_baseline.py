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

from gist_amd import ist
# (dist: the process group setup() opens and main_family ends)
from gist_amd.scripts.cluster_gcn_ist_distrib import add_family_args, add_ist_args, dist, main_family, report_family, setup

FAMILY = ist.DistributedBaselineGCNWrapper        # its facts are the choices of --host-path and --eval-path


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
    if args.use_pp:
        raise SystemExit('gist_amd: --use-pp is not offered for the BaselineGCN family (a GraphConv layer reads h alone, '
                         'there is no [X | A^X] input to precompute)')
    if args.cuda_id < 0:
        raise SystemExit('gist_amd: the BaselineGCN family runs on a GPU (--cuda-id >= 0)')
    # (the wrapper and the loop as gist_amd.ist has them now: a stand-in there is what runs)
    return main_family(args, dataset, log, setup, ist.DistributedBaselineGCNWrapper, ist.train_baseline_gcn, report, comm=comm)


if __name__ == '__main__':
    os.environ.setdefault('GIST_GC_FREEZE', '1')      # this process is the application: sampler.freeze_setup_objects
    main()
