"""What the HIP launchers refuse, by exception type and text.

The launchers of `_ss_hip` validate their arguments before their first HIP
call, and the module imports without a device, so these refusals are checked
on any machine: every call below passes null (or dummy) pointers and must be
turned away before anything is launched.  n > 0 / P > 0 throughout, so the
empty-call early returns are not what is tested.
"""
import pytest

from swiftsnails_amd._native import hip

SGD, ADAGRAD = 0, 1
PTR = 8  # a non-null "pointer" no refused call ever dereferences


@pytest.fixture(scope="module")
def h():
    return hip()


def scalar_table(h, **kw):
    """16-byte [w | h | key] slots, as the fused sparse-LR path uses"""
    return h.DevTable(base=0, cap=1024, stride=16, key_off=8, dim=1, width=2, **kw)


def bf16_table(h):
    return h.DevTable(base=0, cap=1024, stride=80, key_off=64, dim=32, width=32, bf16=1)


def bd_reduce(h, **kw):
    return h.bd_reduce(8, 1, 0, 0, 0, 0, 0, 1, 0, 0, **kw)


def rec_grad(h, nd=1, **kw):
    return h.rec_grad(0, nd, 16, 0, 0, 0, 1, 0, 0, **kw)


def srv_merge(h, D, **kw):
    return h.srv_merge(1, 0, 0, 0, 0, 0, 0, 0, D, **kw)


def pull_unique_bk(h, t, G, **kw):
    return h.pull_unique_bk(t, 0, 0, 0, 0, 1, 0, 0, h.InitParams(), 0, 0, G, 0, **kw)


CASES = {
    "bd_reduce_fused_rule": (
        lambda h: bd_reduce(h, t=scalar_table(h), slots=PTR, op=h.OptParams(kind=SGD)),
        RuntimeError,
        "bd_reduce: fused apply needs scalar AdaGrad or FTRL (z, n) rows and compact ids"),
    "bd_reduce_fused_compact_ids": (
        lambda h: bd_reduce(h, osi=1, t=scalar_table(h), slots=PTR,
                            op=h.OptParams(kind=ADAGRAD)),
        RuntimeError,
        "bd_reduce: fused apply needs scalar AdaGrad or FTRL (z, n) rows and compact ids"),
    "bd_reduce_fused_slot32_rule": (
        lambda h: bd_reduce(h, t=scalar_table(h), slots=PTR, slot32=1,
                            op=h.OptParams(kind=SGD)),
        RuntimeError,
        "bd_reduce: fused apply needs scalar AdaGrad or FTRL (z, n) rows and compact ids"),
    "bd_reduce_keys_without_snapshot": (
        lambda h: bd_reduce(h, t=scalar_table(h), slots=PTR, op=h.OptParams(kind=ADAGRAD),
                            bkeys=PTR),
        RuntimeError,
        "bd_reduce: slot stores with keys need a snapshot merge into 16-byte [w|h|key] slots"),
    "bd_reduce_keys_without_slots": (
        lambda h: bd_reduce(h, bkeys=PTR, snap=PTR),
        RuntimeError,
        "bd_reduce: slot stores with keys need a snapshot merge"),
    "bd_reduce_loss_handoff": (
        lambda h: bd_reduce(h, acc=PTR),
        RuntimeError, "bd_reduce: loss hand-off needs its output"),
    "bd_reduce_loss_handoff_count": (
        lambda h: bd_reduce(h, acc=PTR, acc_out=PTR, acc_n=0),
        RuntimeError, "bd_reduce: loss hand-off needs its output"),
    "bd_reduce_F": (
        lambda h: h.bd_reduce(8, 1, 0, 0, 0, 0, 0, 0, 0, 0),
        RuntimeError, "bd_reduce: F must be >= 1"),
    "srv_merge_fused_rule": (
        lambda h: srv_merge(h, 1, t=scalar_table(h), slots=PTR, op=h.OptParams(kind=SGD)),
        RuntimeError, "bd_reduce_p: fused apply needs scalar AdaGrad or FTRL (z, n) rows"),
    "srv_merge_keys_without_snapshot": (
        lambda h: srv_merge(h, 1, t=scalar_table(h), slots=PTR, op=h.OptParams(kind=ADAGRAD),
                            bkeys=PTR),
        RuntimeError,
        "bd_reduce_p: slot stores with keys need a snapshot merge into [w|h|key] slots"),
    "srv_merge_slot32_wide": (
        lambda h: srv_merge(h, 2, slot32=1),
        ValueError, "srv_merge: slot32 / bkeys are for scalar rows"),
    "srv_merge_rows_table": (
        lambda h: srv_merge(h, 2, t=scalar_table(h), slots=PTR, op=h.OptParams(kind=SGD)),
        RuntimeError, "srv_merge_rows: a fused update needs the table of these rows"),
    "srv_merge_rows_nothing_to_write": (
        lambda h: srv_merge(h, 2),
        RuntimeError, "srv_merge_rows: merged rows or a fused update"),
    "pull_claim_no_regions": (
        lambda h: h.pull_claim_bk(scalar_table(h), 0, 0, 0, 0, 1, PTR, PTR, PTR, h.InitParams(),
                                  0, 0, 0),
        ValueError, "claimed pulls: a region table"),
    "commit_claims_no_regions": (
        lambda h: h.commit_claims(scalar_table(h), 0, 0, 0, 0, 1, PTR, PTR, 0),
        ValueError, "claimed pulls: a region table"),
    "pull_claim_buffers": (
        lambda h: h.pull_claim_bk(scalar_table(h, rbits=2), 0, 0, 0, 0, 1, 0, PTR, PTR,
                                  h.InitParams(), 0, 0, 0),
        ValueError, "claimed pull: slots, rows (or occurrence rows + luid), snapshot"),
    "pull_snapshot_bf16": (
        lambda h: pull_unique_bk(h, bf16_table(h), 1, snap=PTR),
        ValueError, "pull snapshot: scalar (w, h) rows with G = 1 only"),
    "pull_slot32_without_snapshot": (
        lambda h: pull_unique_bk(h, scalar_table(h), 1, slot32=1),
        ValueError, "pull: 4-byte slots need snapshot 16-byte slots, cap < 2^31"),
    "pull_lane_group": (
        lambda h: pull_unique_bk(h, scalar_table(h), 3),
        RuntimeError, "unsupported lane-group size"),
    "probe_lane_group": (
        lambda h: h.probe(scalar_table(h), 0, h.SegList.from_host([0], [8]), 8, 0,
                          h.InitParams(), 0, 0, 0, 8, 0),
        RuntimeError, "unsupported lane-group size"),
    "rec_grad_layout": (
        lambda h: rec_grad(h, nd=0),
        RuntimeError, "rec_grad: bad layout"),
    "rec_grad_loss_handoff": (
        lambda h: rec_grad(h, acc=PTR),
        RuntimeError, "rec_grad: loss hand-off needs its output"),
    "rec_grad_skip": (
        lambda h: rec_grad(h, skip=1),
        RuntimeError, "rec_grad: skipped destination out of range"),
    "bd_reduce_fm_dim": (
        lambda h: h.bd_reduce_fm(8, 1, 0, 0, 0, 0, 0, 2, 3, 0, 0, 0, ovf=0),
        RuntimeError, "bd_reduce_fm: dim must be 1+K with K in {1,4,8,16}"),
    "fm_fwd_g_dim": (
        lambda h: h.fm_fwd_g(PTR, [], 0, 8, 8, 3, 0, 0, 0, 0, 0, 0),
        RuntimeError, "fm_fwd_g: dim must be 1+K with K in {1,4,8,16}"),
    "fm_fwd_bwd_dim": (
        lambda h: h.fm_fwd_bwd(0, 0, 8, 8, 3, 0, 0, 0, 0, 0),
        RuntimeError, "fm_fwd_bwd: dim must be 1+K with K in {1,4,8,16}"),
    "ffm_K": (
        lambda h: h.ffm_fwd_bwd(0, 0, 8, 8, 3, 0, 0, 0, 0, 0),
        RuntimeError, "ffm_fwd_bwd: K must be 2, 4 or 8"),
    "w2v_oreduce_dim": (
        lambda h: h.w2v_oreduce(0, 8, 0, 0, 0, 8, 2, 48, 0, 0),
        RuntimeError, "w2v_oreduce: D must be 32, 64 or 128"),
    "w2v_oreduce_fused_rows": (
        lambda h: h.w2v_oreduce(0, 8, 0, 0, 0, 8, 2, 32, 0, 0, t=scalar_table(h), slots=PTR,
                                op=h.OptParams(kind=SGD)),
        RuntimeError, "w2v_oreduce: a fused update needs aligned rows of this D"),
    "w2v_oreduce_handoff": (
        lambda h: h.w2v_oreduce(0, 8, 0, 0, 0, 8, 2, 32, 0, 0, acc=PTR),
        RuntimeError, "w2v_oreduce: accumulator hand-off needs acc_out"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refused_before_any_launch(h, case):
    call, exc, text = CASES[case]
    with pytest.raises(exc) as e:
        call(h)
    assert type(e.value) is exc
    assert str(e.value).startswith(text), str(e.value)
