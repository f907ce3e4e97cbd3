"""The record exchange's bucket layout (bdedup.hip, the kBdRecLayout bit of a
deduper's layout argument; host-side layout functions, no GPU): a source's
bucket holds 3584 / N records so that server bucket k — the union of the N
sources' bucket k — holds about one one-rank bucket (~3584 records, the
one-GPU dedup's tuned size), up to the bucket-count cap; the unique-key layout
is unchanged by the bit's existence, and the scratch is sized for the layout
a deduper will actually use."""
import pytest

from swiftsnails_amd._native import hip

N_BENCH = 262144 * 39


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_record_layout_server_bucket_size(world):
    h = hip()
    bit = h.bd_record_layout_bit()
    P = h.bd_buckets(N_BENCH, world, world | bit)
    assert P % world == 0
    server_bucket = world * N_BENCH / P  # records of N sources per server bucket
    if world <= 4:
        assert 3400 < server_bucket < 3700, server_bucket
    else:  # the 16K bucket cap: ~5000 records, ~2000 distinct keys at the bench shape
        assert P <= 16384 + 64 and server_bucket < 6000, (P, server_bucket)
    # the layout helpers all see the bit: offsets / scratch agree with the count
    assert h.bd_offsets(N_BENCH, world, world | bit)[0] == P
    assert h.bd_scratch_words(N_BENCH, world, world | bit) > P


def test_unique_layout_unchanged_by_the_bit():
    h = hip()
    bit = h.bd_record_layout_bit()
    # one rank: the same layout either way (no servers merging sources)
    assert h.bd_buckets(N_BENCH, 1, 1 | bit) == h.bd_buckets(N_BENCH, 1, 1)
    # N > 1 unique keys: ~3072 occurrences per source bucket (SS_BD_TARGET_DIST), split
    # by the servers into sub-buckets of a table's size
    tg = h.bd_target_dist()
    for world in (2, 4, 8):
        P = h.bd_buckets(N_BENCH, world, world)
        assert 0.9 * tg < N_BENCH / P < 1.1 * tg
        m = h.srv_sub_buckets(world)
        assert world * (N_BENCH / P) * 1.25 / m <= 3000  # <= ~3000 keys per server table



@pytest.mark.gpu
def test_record_deduper_has_no_server_sub_buckets():
    """A record-layout deduper routes whole buckets: server sub-buckets
    (msub = 2) are refused by split_for_servers and, forced past it, by the
    launcher's host-side check before any launch; with msub = 1 the same call
    puts every occurrence's key and index at its send-segment position."""
    import numpy as np
    import torch

    from swiftsnails_amd.ops.dedup import Deduper
    from swiftsnails_amd.parallel.router import HashFrag

    dev, nranks, n = torch.device("cuda", 0), 2, 4096
    hf = HashFrag(nranks, 97)
    d = Deduper(n, nranks=nranks, frag_map=torch.from_numpy(hf.rank_map().astype(np.int32)),
                device=dev, record_layout=True)
    d.lay_n = n
    d.enable_records()
    k = np.random.default_rng(5).integers(0, 1500, size=n, dtype=np.int64)
    keys = torch.from_numpy(k).to(dev)
    with pytest.raises(RuntimeError, match="split_for_servers: the record layout"):
        d.split_for_servers(2)
    d.msub = 2
    d.usub = torch.zeros(2 * hip().bd_buckets(n, nranks, d.ndest), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="bdedup: the record exchange needs"):
        d(keys)
    d.msub, d.usub = 1, None
    r = d(keys)
    torch.cuda.synchronize()
    d.check()
    # every occurrence j: its key and j at position pos_of[j] of its destination's segment
    pos = d.pos_of.cpu().numpy().view(np.uint32).astype(np.int64)[:n]
    assert len(np.unique(pos)) == n
    np.testing.assert_array_equal(r.ukeys.cpu().numpy()[pos], k)
    np.testing.assert_array_equal(d.spj.cpu().numpy().view(np.uint32)[pos], np.arange(n))
    dest = hf.rank_map()[hf.frag_of(k)]
    np.testing.assert_array_equal(pos // d.ucap, dest)
    uc = r.ucount.cpu().numpy()
    np.testing.assert_array_equal(uc, np.bincount(dest, minlength=nranks))
    assert (pos % d.ucap < uc[dest]).all()
