"""TEST INFRASTRUCTURE (not product): one rank of GIST for the GAT family in its own process on the box's one GPU,
with the product block movers (HipBlocks) and the collective host-staged over gloo (tests/host_staged_comm.py).
Runs tests/gat_ist_restatement.check_round and writes {errors, base (sha256 of every config's final base arena)}.

    python tests/ist_gat_worker.py RANK S PORT OUT.json"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import argparse
    import torch
    import torch.distributed as dist
    from gist_amd import ist
    from tests.gat_ist_restatement import base_init_for, check_round
    from tests.host_staged_comm import HostStagedComm
    rank, S, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    errs, hashes = [], []
    try:
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(dev)
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        H, fin, ncls = 16, 12, 5
        for ci, (L, nh) in enumerate([(1, 4), (3, 3)]):
            args = argparse.Namespace(num_subnet=S, n_hidden=H, n_layers=L, n_heads=nh, rank=rank)
            base_init = base_init_for(ist.gat_dims(fin, H, ncls, L, nh), 200 + ci)
            w = ist.DistributedGATWrapper(args, None, fin, ncls, dev, base_init=base_init if rank == 0 else None,
                                          comm=HostStagedComm())

            def all_base():
                o = [torch.empty(w.base.numel) for _ in range(S)]
                dist.all_gather(o, w.base.params.cpu())
                return o
            errs += ['L=%d nh=%d: %s' % (L, nh, e) for e in check_round([w], S, H, L, base_init, 11 + ci, all_base)]
            torch.cuda.synchronize()
            hashes.append(hashlib.sha256(w.base.params.cpu().numpy().tobytes()).hexdigest())
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        errs.append('EXC ' + repr(e) + traceback.format_exc())
    with open(out, 'w') as f:
        json.dump({'errors': errs, 'base': hashes}, f)


if __name__ == '__main__':
    main()
