"""In-place eviction against the only other way to drop keys, on one GPU.

A sparse-LR shard (16-byte slots) of ``--slots`` slots at load ``--load``;
half of its keys were never pushed (h = 0) and the rule ``acc_below = 0``
removes exactly those.  Interleaved A/B pairs on the same starting bytes (the
table is restored from a copy before every trial, outside the timed window):

  A  ``table.evict(rule)``: mark + cluster repair in place (csrc/hip/evict.hip)
  B  rebuild: ``export`` every row to device buffers, filter in torch, a
     fresh allocation, ``assign`` the survivors (what ``resize`` does)

Times are host clocks around work that ends in a device synchronise; the peak
extra memory is ``torch.cuda.max_memory_allocated`` over the call, above what
was allocated before it; bytes are computed from the shapes.  Both must leave
the same keys and rows.  Prints one JSON line.

    python tools/evict_bench.py [--slots 67108864] [--load 0.5] [--pairs 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main(argv=None):
    from swiftsnails_amd.ops.optim import EvictRule, InitConfig, Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 26)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t = HbmTable(1, a.slots, optimizer=Optimizer("adagrad", lr=0.05), init=InitConfig("zero"),
                 device=dev)
    cap, n = t.capacity, int(a.load * t.capacity)
    step = 1 << 24
    for i in range(0, n, step):  # distinct keys, well mixed by the table hash
        k = torch.arange(i + 1, min(n, i + step) + 1, dtype=torch.int64, device=dev) * 7919
        t.pull(k)
        hot = k[::2].contiguous()
        t.push(hot, torch.ones(hot.numel(), 1, device=dev))
    torch.cuda.synchronize()
    t.check()
    assert t.size() == n
    start = (t.storage.clone(), t.size_ctr.clone())
    rule = EvictRule(acc_below=0.0)

    def restore():
        t.storage.copy_(start[0])
        t.size_ctr.copy_(start[1])
        torch.cuda.synchronize()

    def in_place():
        return t.evict(rule)

    def rebuild():
        chunks = []
        for k, r in t.export(to_host=False):
            keep = r[:, 1] > 0
            chunks.append((k[keep], r[keep]))
        old = t.storage
        t._alloc(cap)
        del old
        for k, r in chunks:
            t.assign(k, r)
        return n - sum(int(k.numel()) for k, _ in chunks)

    def timed(fn):
        restore()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        gone = fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return el, torch.cuda.max_memory_allocated(dev) - base, gone

    def model():
        ks, rs = [], []
        for k, r in t.export(to_host=False):
            ks.append(k)
            rs.append(r)
        k, r = torch.cat(ks), torch.cat(rs)
        o = torch.argsort(k)
        return k[o], r[o]

    res = {"A": [], "B": []}
    for name, fn in (("A", in_place), ("B", rebuild)):  # warm up both, and compare the results
        _, _, gone = timed(fn)
        assert gone == n // 2 and t.size() == n - gone, (name, gone, t.size())
        t.check()
        res[name + "_model"] = model()
    same = all(torch.equal(x, y) for x, y in zip(res.pop("A_model"), res.pop("B_model")))
    for _ in range(a.pairs):
        for name, fn in (("A", in_place), ("B", rebuild)):
            el, mem, _ = timed(fn)
            res[name].append((el, mem))
    ms = lambda xs: [round(1e3 * x[0], 3) for x in xs]  # noqa: E731
    slot, survivors, victims = t.stride, n - n // 2, n // 2
    out = {
        "slots": cap, "table_bytes": cap * slot, "keys": n, "evicted": victims,
        "same_keys_and_rows": bool(same),
        "evict_ms": ms(res["A"]), "evict_ms_median": round(1e3 * statistics.median(
            x[0] for x in res["A"]), 3),
        "rebuild_ms": ms(res["B"]), "rebuild_ms_median": round(1e3 * statistics.median(
            x[0] for x in res["B"]), 3),
        "evict_peak_extra_bytes": max(x[1] for x in res["A"]),
        "rebuild_peak_extra_bytes": max(x[1] for x in res["B"]),
        # bytes from the shapes: the mark pass reads every slot and writes a
        # flag byte, the repair reads the flags (its own and the slot before)
        # and rewrites the victims' slots (moved survivors not counted)
        "evict_bytes_min": cap * slot + 3 * cap + victims * slot,
        # export reads every slot and writes (key, fp32 row) per key; the
        # filter reads those and writes the survivors; the fresh allocation is
        # filled; assign reads the survivors and writes their slots
        "rebuild_bytes_min": cap * slot + n * (8 + 4 * t.width) * 2
        + survivors * (8 + 4 * t.width) * 2 + cap * slot + survivors * slot,
        "one_pass_bytes": cap * slot,
        "one_pass_floor_ms_at_6.3TBps": round(1e3 * cap * slot / 6.3e12, 3),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
