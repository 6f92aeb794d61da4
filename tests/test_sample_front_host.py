"""Host side of the sampler's front end (no GPU, CPU tensors): the refusals of the four sample entries with the texts the GPU tests
match, in the order they are raised; the one-segment verdicts against the expressions sample / sample_tied computed inline before
the entries shared a front end; the whole-axis chunk tuples. T = 12 as two proteins of 5 and 7, N = 3."""
import re

import numpy as np
import pytest
import torch

OFFSETS = [0, 5, 12]
T, N = 12, 3
ENTRIES = ["sample", "sample_tied", "sample_each", "sample_tied_each"]


def valid(what, seed=0):
    """Arguments every entry accepts: an order that stays inside its protein, every step closing."""
    rng = np.random.default_rng(seed)
    order = np.stack([np.concatenate([a + rng.permutation(b - a) for a, b in zip(OFFSETS, OFFSETS[1:])]) for _ in range(N)])
    return dict(order=order, close=np.ones((N, T), np.int32) if "tied" in what else None, S_fixed=rng.integers(0, 21, (N, T)),
                free=np.ones((N, T), np.float32), u=rng.random((N, T)).astype(np.float32), temperature=0.5, weight=None, bias=None,
                allowed=None, pssm_mix=None, pssm_bias=None, pssm_keep=None)


def front(what, offsets=OFFSETS, **changed):
    """Steps 1-4 as Engine._sample_front runs them: the arguments, then the verdicts (the whole-axis entries pass no offsets)."""
    from thermompnn_amd.engine import sample_args, sample_verdicts
    rows, tabs, res = sample_args(what, T, torch.device("cpu"), **dict(valid(what), **changed))
    each = what.endswith("_each")
    offs = sample_verdicts(what, rows["order"], rows["S_fixed"], rows["close"], torch.tensor(offsets, dtype=torch.int32) if each else None)
    return rows, tabs, res, offs


def refused(what, text, **changed):
    from thermompnn_amd._lib import TmpnnError
    with pytest.raises(TmpnnError, match=re.escape(text)) as e:
        front(what, **changed)
    assert str(e.value).startswith(f"{what}: ")
    return str(e.value)


def changed_at(a, index, value):
    a = np.array(a)
    a[index] = value
    return a


@pytest.mark.parametrize("what", ENTRIES)
def test_valid_arguments_pass(what):
    rows, tabs, res, offs = front(what, bias=np.zeros((T, 21)), allowed=np.ones((T, 21)))
    assert offs == (OFFSETS if what.endswith("_each") else [0, T])
    assert [rows[k].dtype for k in ("order", "S_fixed", "free", "u")] == [torch.int32, torch.int32, torch.float32, torch.float32]
    assert (rows["close"] is not None and rows["close"].dtype == torch.int32) == ("tied" in what) and rows["weight"] is None
    assert tabs["bias"].dtype == torch.float32 and tabs["pssm_mix"] is None and list(tabs) == ["bias", "allowed", "pssm_mix", "pssm_bias", "pssm_keep"]
    assert res["S"].shape == (N, T) and res["S"].dtype == torch.int32 and res["probs"].shape == (N, T, 21)
    empty = front(what, **{k: np.zeros((0, T)) for k in ("order", "S_fixed", "free", "u")}, **({"close": np.zeros((0, T))} if "tied" in what else {}))
    assert empty[2]["S"].shape == (0, T) and empty[2]["probs"].shape == (0, T, 21)


@pytest.mark.parametrize("what", ENTRIES)
def test_refusals_of_the_arguments(what):
    v = valid(what)
    assert "u must be [N, 12] like order" in refused(what, "order", u=v["u"][:, :11])            # a short u: a shape error naming order
    refused(what, "like order", S_fixed=v["S_fixed"][:2])
    refused(what, "like order", free=v["free"][0])
    for t in (0.0, -1.0, float("inf"), float("nan")):
        refused(what, "temperature", temperature=t)
    refused(what, "bias must be", bias=np.zeros((5, 21), np.float32))
    refused(what, "allowed must be", allowed=np.zeros((T, 20), np.float32))
    twice = changed_at(v["order"], (1, 5), v["order"][1, 6])
    refused(what, "bias must be", order=twice, bias=np.zeros((5, 21), np.float32))               # a wrong bias shape: before any verdict
    refused(what, "like order", u=v["u"][:, :11], temperature=0.0)                              # shapes, then the temperature
    refused(what, "temperature", temperature=0.0, bias=np.zeros((5, 21), np.float32))           # the temperature, then the tables
    if "tied" in what:
        assert "close must be [N, 12]" in refused(what, "like order", close=v["close"][:, :11])
        assert "weight must be [N, 12]" in refused(what, "like order", weight=np.ones((1, T), np.float32))
        refused(what, "pssm_keep must be [12, 21]", pssm_keep=np.ones((T, 20), np.float32))
        refused(what, "pssm_mix must be [12]", pssm_mix=np.ones((11,), np.float32), pssm_bias=np.ones((T, 21), np.float32))
        refused(what, "pssm_bias must be [12, 21]", pssm_mix=np.ones((T,), np.float32), pssm_bias=np.ones((T, 20), np.float32))
        refused(what, "pssm_bias goes with pssm_mix", pssm_bias=np.ones((T, 21), np.float32))
        refused(what, "pssm_bias goes with pssm_mix", pssm_mix=np.ones((T,), np.float32))
        refused(what, "pssm_bias goes with pssm_mix", pssm_mix=np.ones((11,), np.float32))       # the pairing, then the shapes
        front(what, weight=np.ones((N, T)), pssm_mix=np.ones(T), pssm_bias=np.ones((T, 21)), pssm_keep=np.ones((T, 21)))


@pytest.mark.parametrize("what", ENTRIES)
def test_refusals_of_the_verdicts(what):
    v = valid(what)
    tied, each = "tied" in what, what.endswith("_each")
    twice = changed_at(v["order"], (1, 5), v["order"][1, 6])
    refused(what, "permutation", order=twice)
    refused(what, "must be a permutation of 0..11", order=v["order"] + 1)
    refused(what, "permutation", order=v["order"] - 1)
    refused(what, "residue indices", S_fixed=changed_at(v["S_fixed"], (0, 0), 21))
    refused(what, "residue indices must lie in [0, 21)", S_fixed=changed_at(v["S_fixed"], (2, 11), -1))
    refused(what, "permutation", order=twice, S_fixed=changed_at(v["S_fixed"], (0, 0), 21))     # the order, then the letters
    outside = np.array(v["order"])
    outside[1, [2, 8]] = outside[1, [8, 2]]                              # still a permutation of 0..11, two entries in the wrong protein
    if each:
        refused(what, "inside the protein", order=outside)
        refused(what, "permutation", order=changed_at(outside, (1, 5), outside[1, 6]))
        refused(what, "inside the protein", order=outside, S_fixed=changed_at(v["S_fixed"], (0, 0), 21))
        for bad in ([0, 5, 11], [1, 5, 12], [0, 7, 5, 12]):
            refused(what, "offsets must rise from 0 to T = 12", offsets=bad)
    else:
        assert front(what, order=outside)[3] == [0, T]                    # the whole axis is one segment
    if tied:
        refused(what, "close must hold 0 or 1", close=changed_at(v["close"], (0, 3), 2))
        refused(what, "close must hold 0 or 1", close=changed_at(v["close"], (1, T - 1), 2))    # 0 / 1, then the last step
        refused(what, "residue indices", S_fixed=changed_at(v["S_fixed"], (0, 0), 21), close=changed_at(v["close"], (0, 3), 2))
        open_end = changed_at(v["close"], (1, T - 1), 0)
        spans = changed_at(v["close"], (1, 4), 0)                         # protein 0's last step stays open
        if each:
            refused(what, "last step must close", close=open_end)
            refused(what, "every protein's last step must close (close[n, offsets[b + 1] - 1] == 1)", close=spans)
        else:
            assert "close" in refused(what, "close[:, -1] must be 1 (the last step ends its group)", close=open_end)
            front(what, close=spans)
        front(what, close=changed_at(v["close"], (slice(None), [0, 1, 5, 6]), 0))


def test_one_segment_verdicts_equal_the_inline_expressions():
    """``each_verdicts`` over one segment against the four expressions of sample / sample_tied, and the refusal ``sample_verdicts``
    raises against the first of them that fails, over draws that break each of them."""
    from thermompnn_amd._lib import TmpnnError
    from thermompnn_amd.engine import VOCAB, each_verdicts, sample_verdicts
    rng = np.random.default_rng(7)
    texts = ["permutation", "residue indices", "close must hold 0 or 1", "close[:, -1] must be 1"]
    seen = {k: 0 for k in ["repeated", "out of range", "letter 21", "letter -1", "close 2", "open end", "all pass", *texts]}
    one = torch.tensor([0, T], dtype=torch.int32)
    for _ in range(300):
        order = np.stack([rng.permutation(T) for _ in range(N)])
        S = rng.integers(0, 21, (N, T))
        close = (rng.random((N, T)) < 0.6).astype(np.int64)
        close[:, -1] = 1
        n, s = int(rng.integers(N)), int(rng.integers(T))
        kinds = [k for k in ("repeated", "out of range", "letter 21", "letter -1", "close 2", "open end") if rng.random() < 0.2]
        for kind in kinds:
            seen[kind] += 1
            if kind == "repeated":
                order[n, s] = order[n, (s + 1) % T]
            elif kind == "out of range":
                order[n, s] = T if rng.random() < 0.5 else -1
            elif kind.startswith("letter"):
                S[n, s] = int(kind.split()[1])
            elif kind == "close 2":
                close[n, s] = 2
            else:
                close[n, -1] = 0
        O, S0, Cl = (torch.as_tensor(a, dtype=torch.int32) for a in (order, S, close))
        steps = torch.arange(T, dtype=torch.int32)
        inline = [bool((torch.sort(O, dim=1).values == steps).all()), bool(((S0 >= 0) & (S0 < VOCAB)).all()),
                  bool(((Cl == 0) | (Cl == 1)).all()), bool((Cl[:, -1] == 1).all())]
        for offsets in (None, one):                                     # the whole-axis entries pass None; [0, T] says the same
            got = each_verdicts(O, S0, Cl, offsets).tolist()
            assert got[1] is True and [got[0], *got[2:]] == inline, (kinds, got, inline)
            assert each_verdicts(O, S0, None, offsets).tolist() == [inline[0], True, inline[1]]
        for what, checks in (("sample", inline[:2]), ("sample_tied", inline)):
            cl = Cl if what == "sample_tied" else None
            if all(checks):
                assert sample_verdicts(what, O, S0, cl, None) == [0, T]
                seen["all pass"] += what == "sample_tied"
            else:
                first = texts[checks.index(False)]
                with pytest.raises(TmpnnError, match=re.escape(first)):
                    sample_verdicts(what, O, S0, cl, None)
                seen[first] += 1
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_whole_axis_chunk_tuples():
    from thermompnn_amd.engine import Engine, plan_axis_chunks
    for n in (1, N, 7):
        for max_rows, per in ((T - 1, 1), (T, 1), (2 * T, 2), (3 * T + 5, 3), (None, (1 << 18) // T)):
            plan = plan_axis_chunks(T, n, max_rows)
            assert per == Engine._per_chunk(max_rows, T)
            assert plan == [(0, 1, n0, min(n, n0 + per)) for n0 in range(0, n, per)]           # the chain ranges of Engine._chunked
            assert all(c[:2] == (0, 1) and c[2] < c[3] for c in plan)
            assert plan[0][2] == 0 and plan[-1][3] == n and all(a[3] == b[2] for a, b in zip(plan, plan[1:]))      # [0, n) once, rising
            assert max(c[3] - c[2] for c in plan) == plan[0][3] - plan[0][2] == min(per, n)
    assert plan_axis_chunks(T, 0, None) == []
    assert len(plan_axis_chunks(T, N, T - 1)) == N and len(plan_axis_chunks(T, N, None)) == 1
