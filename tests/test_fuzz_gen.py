"""The fuzz generators of tests/_fuzz_gen.py on the CPU models alone (no GPU): the default seeds must not degenerate
into trivial batches — the shares below are conditions on the generators, not measurements of the library — and the
model-level round trip must hold on every receive-coalescing case: coalesce (tests/_gro.py, tests/_gro_flow.py),
expand (tests/_tso.py), and every frame the transmit pass made comes back byte for byte."""
import functools

import numpy as np
import pytest

import _fuzz_gen as Z
import _gro
import _gro_flow
import _tso
import _tx

GRO_CASES, TSO_CASES, TX_CASES = range(Z.GRO_CASES), range(Z.TSO_CASES), range(Z.TX_CASES)


@functools.lru_cache(maxsize=None)
def _gro_case(case):
    ipver, buf, offs, valid, untouched = Z.gro_batch(case)
    return ipver, buf, offs, valid, untouched, _gro.gro(buf, offs, valid, ipver), \
        _gro_flow.gro_flow(buf, offs, valid, ipver)


def _share(hits, cases):
    return sum(bool(h) for h in hits), len(cases)


def test_generators_are_pure_functions_of_the_case():
    a, b = Z.gro_batch(7), Z.gro_batch(7)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    (p, po, pn), (q, qo, qn) = Z.tso_batch(5), Z.tso_batch(5)
    assert np.array_equal(p.sup.data, q.sup.data) and np.array_equal(p.mss, q.mss) and np.array_equal(po, qo) and pn == qn
    c, e = Z.tx_batch(3), Z.tx_batch(3)
    assert np.array_equal(c.data, e.data) and np.array_equal(c.out_off, e.out_off) and c.null == e.null


def test_gro_batches_stay_within_their_bounds():
    for case in GRO_CASES:
        ipver, buf, offs, valid, untouched, _, _ = _gro_case(case)
        n = offs.size - 1
        assert ipver == (4 if case % 2 == 0 else 6) and 1 <= n <= 12 * 24
        assert valid.shape == untouched.shape == (n,) and valid.dtype == untouched.dtype == np.bool_
        assert 0 <= int(offs[0]) <= 3 and int(offs[-1]) + 3 == buf.size <= (1 << 20) + 16
        assert (np.diff(offs.astype(np.int64)) >= 0).all()


def test_gro_batches_hold_runs():
    got, of = _share([max(o["frame_cnt"].max(initial=0), g["frame_cnt"].max(initial=0)) >= 2
                      for *_, o, g in map(_gro_case, GRO_CASES)], GRO_CASES)
    assert 4 * got >= 3 * of, (got, of)


def test_gro_batches_hold_non_members():
    got, of = _share([(o["frame_seg"] == _gro.NONE).any() for *_, o, _ in map(_gro_case, GRO_CASES)], GRO_CASES)
    assert 2 * got >= of, (got, of)


def test_gro_batches_where_the_flow_key_merges_more():
    got, of = _share([g["n_super"] < o["n_super"] for *_, o, g in map(_gro_case, GRO_CASES)], GRO_CASES)
    assert 3 * got >= of, (got, of)


def test_gro_batches_hold_frames_past_one_row_pair():
    """A frame longer than 2,148 bytes: more than 2 KiB of payload behind IPv6 and TCP headers with 40 option bytes."""
    got, of = _share([np.diff(offs.astype(np.int64)).max() > 2148 for _, _, offs, *_ in map(_gro_case, GRO_CASES)],
                     GRO_CASES)
    assert 3 * got >= of, (got, of)


def test_gro_batches_draw_every_profile_and_mutation():
    """Over the default seeds: every mss of the set, every option length, every delivery-independent property the
    generator promises shows up at least once."""
    pays, optb, ctl, trunc, cleared, wraps = set(), set(), 0, 0, 0, 0
    for case in GRO_CASES:
        ipver, buf, offs, valid, untouched, o, _ = _gro_case(case)
        pays |= set(np.diff(o["data_off"]).tolist()) | set(o["mss"].tolist())
        optb |= set(np.diff(o["opt_off"]).tolist())
        ctl |= int(np.bitwise_or.reduce(o["control"], initial=0))
        trunc += int((np.diff(offs.astype(np.int64)) < _tx.IPH[ipver] + 20).sum())
        cleared += int((~valid).sum())
        wraps += int((o["seq_num"].astype(np.uint64) + np.diff(o["data_off"]) >= 1 << 32).sum())
    assert {1, 3, 7, 536, 1448, 1460, 1461, 2040, 2049, 4100, 8948, 8960} <= pays
    assert {0, 4, 12, 40} <= optb
    assert ctl & _gro.CWR and ctl & _gro.FIN and ctl & _gro.PSH
    assert trunc and cleared and wraps


@pytest.mark.parametrize("flow", [False, True], ids=["adjacent", "flow"])
def test_gro_model_round_trip(flow):
    """as_batch(gro(...)) expanded by tests/_tso.expected gives back every untouched member frame byte for byte, at
    its own length; keyed by flow, output position p is input frame order[p]."""
    frames = 0
    for case in GRO_CASES:
        ipver, buf, offs, valid, untouched, o, g = _gro_case(case)
        out = g if flow else o
        if out["n_super"] == 0:
            continue
        b = _gro.as_batch(out, ipver)
        built, _, c = _tso.expected(b)
        member = out["frame_seg"] != _gro.NONE
        pos = out["order"][:b.nf] if flow else np.nonzero(member)[0]
        assert pos.size == b.nf and member[pos].all()
        for p, f in enumerate(pos):
            if untouched[f]:
                src = buf[int(offs[f]):int(offs[f + 1])]
                assert int(c.flen[p]) == src.size, (case, p, f)
                assert np.array_equal(built[int(b.off[p]):int(b.off[p]) + src.size], src), (case, p, f)
                frames += 1
    assert frames > 1000


@functools.lru_cache(maxsize=None)
def _tso_case(case):
    b, off, null = Z.tso_batch(case)
    return b, off, null, _tso.expand(b, null)


def test_tso_batches_stay_within_their_bounds():
    for case in TSO_CASES:
        b, off, null, c = _tso_case(case)
        lens = np.diff(b.sup.data_off)
        assert 1 <= b.n <= 200 and lens.max() <= 70_000 and lens.sum() <= (2 << 20) + 70_000
        assert set(b.mss.tolist()) <= set(Z.TSO_MSS) and set(null) <= set(Z.NULLABLE)
        assert off.size == b.nf + 1 and not (off % 4).any() and (np.diff(off) >= np.diff(b.off)).all()
        assert int(off[0]) <= 12 and int((np.diff(off) - np.diff(b.off)).max(initial=0)) <= 60


def test_tso_batches_hold_multi_frame_super_segments():
    got, of = _share([np.diff(b.first).max() >= 2 for b, *_ in map(_tso_case, TSO_CASES)], TSO_CASES)
    assert 4 * got >= 3 * of, (got, of)


def test_tso_batches_hold_frames_that_cannot_be_built():
    got, of = _share([(c.wire > _tx.WIRE_MAX[b.ipver]).any() for b, _, _, c in map(_tso_case, TSO_CASES)], TSO_CASES)
    assert 8 * got >= of, (got, of)


def test_buildable_variants_hold_no_frame_that_cannot_be_built():
    """The host calls refuse a batch with such a frame: their fuzz cases then take the buildable draw, which must
    still hold frames of more than 60,000 bytes."""
    longest = 0
    for case in TSO_CASES:
        b, off, null = Z.tso_batch(case, buildable=True)
        c = _tso.expand(b, null)
        assert (c.wire <= _tx.WIRE_MAX[b.ipver]).all() and off.size == b.nf + 1
        longest = max(longest, int(c.flen.max()))
    for case in TX_CASES:
        c = Z.tx_batch(case, buildable=True)
        assert (c.wire <= _tx.WIRE_MAX[c.ipver]).all()
        longest = max(longest, int(c.flen.max()))
    assert longest > 60_000


def test_tso_and_tx_batches_draw_every_layout():
    """Over the default seeds of both: batches with and without an option array, every option set, gapped and packed
    slots, every optional array passed as NULL at least once, and for tx a frame past the IP length field."""
    for cases in ([_tso_case(k)[:3] for k in TSO_CASES],
                  [(c, c.out_off, c.null) for c in map(Z.tx_batch, TX_CASES)]):
        packed = [np.array_equal(off - off[0], (b.off if hasattr(b, "sup") else b.packed())) and off[0] == 0
                  for b, off, _ in cases]
        assert any(packed) and not all(packed)
        arrays = [(b.sup if hasattr(b, "sup") else b).opt_off for b, _, _ in cases]
        assert any(a is None for a in arrays) and any(a is not None for a in arrays)
        lens = set().union(*[set(np.diff(a).tolist()) for a in arrays if a is not None])
        assert {0} | {len(_tx.opt_bytes(np.random.default_rng(0), k)) for k in _tx.OPT_SETS} <= lens
        assert set().union(*[set(null) for _, _, null in cases]) == set(Z.NULLABLE)
    over = [(c.wire > _tx.WIRE_MAX[c.ipver]).sum() for c in map(Z.tx_batch, TX_CASES)]
    assert sum(o > 0 for o in over) >= 3 and max(int(c.flen.max()) for c in map(Z.tx_batch, TX_CASES)) > 60_000
