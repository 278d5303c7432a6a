"""CPU tests of bench.py's multi-GPU plumbing (gloo, world_size 2): the only
collectives (MAX time, SUM frames) and the LPT sharding of config 5."""
import os
import socket
import sys

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        el, fr = bench.reduce_over_ranks(dist, 1.0 + rank, 100 * (rank + 1))
        bad = bench.sum_over_ranks(dist, rank + 1)
        q.put((rank, el, fr, bad))
    finally:
        dist.destroy_process_group()


def test_reduce_over_ranks_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, el, fr, bad in res:
        assert el == 2.0  # max over ranks
        assert fr == 300  # sum over ranks
        assert bad == 3  # output-check counters summed over ranks


def test_reduce_over_ranks_single():
    assert bench.reduce_over_ranks(None, 1.5, 7) == (1.5, 7)


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_shard_lpt_balanced_and_complete(world):
    costs = [((i * 7919) % 97) + 1.0 for i in range(1000)]
    parts = bench.shard_lpt(costs, world)
    assert sorted(i for p in parts for i in p) == list(range(1000))
    loads = [sum(costs[i] for i in p) for p in parts]
    assert max(loads) - min(loads) <= max(costs)


def _mixed_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # configs[4]: 65,536 stills over `world` GPUs, per-GPU --frames = 65536 / world
        mine, items = bench.rank_batch("mixed", 65536 // world, world, rank)
        shards = [None] * world
        dist.all_gather_object(shards, mine)
        cost = sum(len(items[i][0]) + 0.02 * items[i][2] for i in mine)
        el, fr = bench.reduce_over_ranks(dist, 10.0 + rank, len(mine))
        q.put((rank, shards, len(items), cost, el, fr))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_mixed_configs4_flow_gloo(world):
    """bench.py's configs[4] flow over the full 65,536-item list: every rank builds the same
    global list, the LPT shards are disjoint and complete, the frame SUM and time MAX are right."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mixed_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shards = res[0][1]
    assert all(r[1] == shards for r in res)  # every rank computed the same partition
    flat = [i for sh in shards for i in sh]
    assert len(flat) == 65536 and sorted(flat) == list(range(65536))
    for rank, sh, total, cost, el, fr in res:
        assert total == 65536
        assert sh[rank] == shards[rank]
        assert el == 10.0 + world - 1  # max over ranks
        assert fr == 65536  # sum over ranks
    costs = [r[3] for r in res]
    assert max(costs) - min(costs) <= 0.01 * max(costs)  # LPT: balanced shards


def test_verify_outputs_against_manifest():
    """bench.py's post-timing output check: every committed bench stream is in the manifest, the
    oracle's own JPEG passes, a flipped byte and an unknown stream are counted."""
    import glob
    import hashlib
    import json
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_py as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    man = json.load(open(os.path.join(root, "tests", "golden", "bench_manifest.json")))
    for wl in bench.WORKLOADS.values():
        if wl["streams"]:
            for f in glob.glob(os.path.join(root, wl["streams"])):
                assert hashlib.md5(open(f, "rb").read()).hexdigest() in man, f
    for pat, *_ in bench.MIXED_SETS.values():
        for f in glob.glob(os.path.join(root, pat)):
            assert hashlib.md5(open(f, "rb").read()).hexdigest() in man, f
    s = open(os.path.join(root, "tests", "golden", "bench264", "avc1080_00.h264"), "rb").read()
    j = O.transcode(s)
    batch = [s, s, b"unknown"]
    out = bytearray(j + j + j)
    offs, lens = [0, len(j), 2 * len(j)], [len(j)] * 3
    assert bench.verify_outputs(batch, out, offs, lens, man) == (3, 0, 1)
    out[len(j) + 100] ^= 1
    assert bench.verify_outputs(batch, out, offs, lens, man) == (3, 1, 1)


def _fake_outputs(n, size):
    """n 'JPEGs' of `size` bytes each, back to back with a gap, picture 2 failed."""
    import ctypes
    stride = size + 7
    out = (ctypes.c_uint8 * (n * stride))()
    offs, lens, status = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    for i in range(n):
        offs[i], lens[i] = i * stride, size
        ctypes.memmove(ctypes.addressof(out) + offs[i], bytes((i * 31 + k) & 255 for k in range(size)), size)
    status[2], lens[2] = -7, 0
    return out, offs, lens, status


def test_dump_outputs_files_sample_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 .npy files, status / length / CRC-32 of every picture, the
    bytes of a seeded sample that respects the byte budget, identical from run to run."""
    import zlib
    import numpy as np
    n, size = 12, 1000
    out, offs, lens, status = _fake_outputs(n, size)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 5 * size + 10)  # room for 5 of the 11 good pictures
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, offs, lens, status, n)
    bench.dump_outputs(str(b), out, offs, lens, status, n)
    names = sorted(os.listdir(a))
    assert names == ["jpeg_crc32.npy", "jpeg_lens.npy", "jpeg_sample_bytes.npy", "jpeg_sample_index.npy",
                     "jpeg_status.npy"]
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    d = {name[:-4]: np.load(a / name) for name in names}
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    raw = bytes(out)
    want_len = [0 if i == 2 else size for i in range(n)]
    assert d["jpeg_status"].tolist() == [-7 if i == 2 else 0 for i in range(n)]
    assert d["jpeg_lens"].tolist() == want_len
    assert d["jpeg_crc32"].tolist() == [zlib.crc32(raw[offs[i]:offs[i] + want_len[i]]) if i != 2 else 0
                                        for i in range(n)]
    idx = [int(i) for i in d["jpeg_sample_index"]]
    assert len(idx) == 5 and idx == sorted(set(idx)) and 2 not in idx
    assert d["jpeg_sample_bytes"].astype(np.uint8).tobytes() == b"".join(raw[offs[i]:offs[i] + size] for i in idx)
    # everything fits: every good picture is dumped
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", n * size)
    bench.dump_outputs(str(a), out, offs, lens, status, n, ".rank1")
    assert np.load(a / "jpeg_sample_index.rank1.npy").tolist() == [i for i in range(n) if i != 2]
