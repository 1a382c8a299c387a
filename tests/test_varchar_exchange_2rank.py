"""Two ranks through rw_exchange_run_typed: the q8 person / auction streams
(person.name a varchar) cross the all-to-all-v, each rank feeds what it
receives to its own GPU join executor, and the union of the two ranks' join
outputs must equal one executor over the unpartitioned stream.

Same adaptive shape as tests/test_dist_gpu.py: subprocess workers, and a
clean SKIP when the communicator refuses one device for two ranks (RCCL
allows one rank per device), which is what happens on a one-GPU machine.
"""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1413


def _worker_main():
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    result_dir = os.environ["RESULT_DIR"]
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ctypes as C

    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    import risingwave_amd
    from rwtest import ffi
    from rwtest import varchar as vc
    from rwtest import xpayload as xp
    from rwtest.varchar import VChunk
    from test_varchar_exchange import (Q8_TYPES, gpu_join, q8_stream,
                                       single_executor_epochs)

    risingwave_amd.load_library()
    exch = bench.setup_exchange(ffi, rank, world, dist)
    if exch is None:
        with open(os.path.join(result_dir, f"refused.{rank}"), "w") as f:
            try:
                f.write(xp.XLib(handle=False).err())
            except Exception as e:  # noqa: BLE001
                f.write(str(e))
        dist.barrier()
        dist.destroy_process_group()
        sys.exit(42)
    xl = xp.XLib(handle=False)
    xl.adopt(exch.h, world)

    # every rank generates the same stream; in step s rank r contributes
    # chunk s * world + r, so receiving in peer order keeps the chunk order
    epochs = q8_stream(SEED, chunks_per_epoch=2 * world)
    cap = 4 << 20
    send, recv = xl.alloc(cap), xl.alloc(cap)
    join = gpu_join()
    outs = []
    for e, chunks in enumerate(epochs):
        rows = []
        for s in range(len(chunks) // world):
            side, ops, crows = chunks[s * world + rank]
            types = Q8_TYPES[side]
            batch = xp.Batch(xl, types,
                             [[r[i] for r in crows] for i in range(3)], ops)
            kc = (C.c_uint32 * 1)(0)
            arrs = [(C.c_uint64 * world)() for _ in range(4)]
            rc = xl.L.rw_exchange_run_typed(
                xl.h, batch.desc, 3, batch.ops, batch.n, kc, 1, 256, send, cap,
                recv, cap, *arrs)
            assert rc == 0, xl.err()
            batch.free()
            r_rows, r_vb = list(arrs[2]), list(arrs[3])
            off = 0
            for p in range(world):
                pside = chunks[s * world + p][0]
                ptypes = Q8_TYPES[pside]
                size = xp.Layout(r_rows[p], 3, r_vb[p]).total
                block = xp.decode_block(xl.download(recv, size, off),
                                        r_rows[p], ptypes, r_vb[p])
                off += size
                if not block:
                    continue
                join.push(pside, VChunk.from_rows(
                    ptypes, [op for op, _ in block],
                    [row for _, row in block]))
                for c in vc.poll_all(join):
                    rows.extend(c.visible_rows())
        join.flush(e + 1)
        outs.append(rows)
    join.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, outs)
    if rank == 0:
        single = single_executor_epochs(epochs)
        with open(os.path.join(result_dir, "result.pkl"), "wb") as f:
            pickle.dump((gathered, single), f)
    dist.barrier()
    dist.destroy_process_group()


def test_typed_exchange_2ranks(tmp_path):
    import torch

    world = 2
    n_dev = max(torch.cuda.device_count(), 1)
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29791",
            "RESULT_DIR": str(tmp_path),
            "HIP_VISIBLE_DEVICES": str(rank % n_dev),
            "RW_VARCHAR_2RANK_WORKER": "1",
        })
        procs.append(subprocess.Popen(
            [sys.executable, os.path.abspath(__file__)], env=env))
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=180))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if all(rc == 42 for rc in rcs):
        err = ""
        for rank in range(world):
            p = tmp_path / f"refused.{rank}"
            if p.exists():
                err = p.read_text()
                break
        pytest.skip("RCCL: one rank per device (clean refusal on a "
                    f"single-GPU box): {err!r}; the R = 1 typed run and the "
                    "partition at 1..64 destinations are covered by "
                    "test_varchar_exchange.py")
    assert all(rc == 0 for rc in rcs), f"worker exit codes {rcs}"

    sys.path.insert(0, os.path.join(REPO, "tests"))
    from rwtest import varchar as vc

    with open(tmp_path / "result.pkl", "rb") as f:
        gathered, single = pickle.load(f)
    for e, want in enumerate(single):
        union = vc.sort_rows(gathered[0][e] + gathered[1][e])
        assert union == want, f"epoch {e}: rank union diverged"
        assert gathered[0][e] and gathered[1][e]


if __name__ == "__main__" and os.environ.get("RW_VARCHAR_2RANK_WORKER"):
    _worker_main()
