"""TEST INFRASTRUCTURE (not product): one rank of gist_amd.ist.train_gat(host_path='engine') in its own process on the
box's one GPU -- the single-site path: the optimiser launch of a step extracts the next batch, across dispatch and sync
boundaries, and check_extract() runs before every evaluation.  The collective is host-staged over gloo
(tests/host_staged_comm.py).  Writes what tests/ist_gat_engine_common.run returns (torch.save) plus `errors`.

    python tests/ist_gat_engine_worker.py RANK S PORT OUT.pt H L HEADS MERGE WEIGHT_DECAY"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from gist_amd import ist
    from tests import ist_gat_engine_common as common
    from tests.host_staged_comm import HostStagedComm
    rank, S, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    H, L, nh, merge, wd = int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7]), sys.argv[8], float(sys.argv[9])
    res = {'errors': []}
    try:
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(dev)
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
        ds = common.dataset()
        it = common.iterator('engine', ds, dev)
        fin, ncls = ds.g.ndata['feat'].shape[1], ds.num_classes
        w = ist.DistributedGATWrapper(common.site_args(S, H, L, nh, merge, wd, rank), None, fin, ncls, dev,
                                      base_init=common.base_init(ds, S, H, L, nh, merge) if rank == 0 else None,
                                      comm=HostStagedComm())
        res.update(common.run('engine', [w], ds, it, dev))
        res['prefetch'] = bool(w.engine.prefetch)
        res['arena_adopted'] = w.engine.arena is w.sub
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        res['errors'].append('EXC ' + repr(e) + traceback.format_exc())
    torch.save(res, out)


if __name__ == '__main__':
    main()
