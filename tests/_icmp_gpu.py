"""Shared helpers of the ICMP GPU tests (tests/test_gpu_icmp_err.py, test_gpu_icmp_rx.py, test_gpu_icmp_echo.py,
test_gpu_icmp_fuzz.py): one device call over outputs pre-filled with a fill byte and held between guard entries, the
model's outputs (tests/_icmp.py) laid into arrays filled the same way, and their comparison array for array — so every
region that must stay untouched is compared too. Also the 4 GiB arena of the far-offset cases (tests/_far.py)."""
import numpy as np
import pytest

import _far
import _gro
import _icmp as M
import _gro_gpu
from _gpu import dev, host, mask_words, setup_gpu, torch, nsx

FILL = 0xAB
GUARD = 64  # fill bytes on either side of a byte buffer handed to a call, inside one device allocation
d = _gro_gpu.d
A4, B4 = bytes([10, 0, 0, 1]), bytes([192, 0, 2, 7])
A6, B6 = bytes([0x20, 1, 0xd, 0xb8] + [0] * 11 + [1]), bytes([0xfe, 0x80] + [0] * 13 + [9])
OUR = {4: A4, 6: A6}
_DT = {"n_out": np.uint64, "out_off": np.uint64, "src_frame": np.uint32, "status": np.uint8}


@pytest.fixture(scope="module")
def arena():
    """2^32 + 8 MiB zeroed device bytes (tests/_far.py), one per test module."""
    setup_gpu()
    a = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def put(arena, pieces):
    arena.zero_()
    for at, b in pieces:
        if len(b):
            arena[at:at + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))


def _all_equal(t, byte):
    n = t.numel()
    a = min((-t.data_ptr()) % 8, n)
    m = (n - a) // 8
    word = int.from_bytes(bytes([byte]) * 8, "little", signed=True)
    ok = bool((t[:a] == byte).all()) and bool((t[a + 8 * m:] == byte).all())
    return ok and (m == 0 or bool((t[a:a + 8 * m].view(torch.int64) == word).all()))


def check_arena(arena, pieces, what=""):
    """The arena holds exactly `pieces`: each window compared on the host, the slices between them still zero."""
    torch.cuda.synchronize()
    at = 0
    for lo, hi in _far.windows(pieces):
        assert _all_equal(arena[at:lo], 0), f"{what}: bytes written in [{at}, {lo}), outside every frame"
        got, want = arena[lo:hi].cpu().numpy(), _far.window_bytes(pieces, lo, hi)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}: {bad.size} bytes differ in [{lo}, {hi}), first at {lo + int(bad[0])}: got "
                                 f"{got[bad[:8]]}, want {want[bad[:8]]}")
        at = hi
    assert _all_equal(arena[at:], 0), f"{what}: bytes written in [{at}, {_far.ARENA})"


def filled(count, dtype):
    """`count` entries of a torch dtype, every byte FILL."""
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(count, 1) * size,), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def words(bits):
    """The mask words of n booleans (one word at least)."""
    w = mask_words(np.asarray(bits).astype(np.uint8))
    return w if w.size else np.zeros(1, np.uint64)


def d_words(bits):
    return d(words(bits))


def bits_of(t, n):
    return _gro.valid_bits(host(t).view(np.uint64), n)


# ------------------------------------------------------------------ error generation
def err_sizes(n, max_out, ipver, nbytes):
    """Entries of every output at its worst-case size, plus one guard entry each."""
    m = min(n, max_out)
    return dict(n_out=2, out_off=m + 2, src_frame=m + 1, status=n + 1), nsx.icmp_err_out_bytes(ipver, n, max_out, nbytes)


def err_gpu(buf, offs, req, arg, ipver, src=None, ttl=64, ident0=0, max_out=None, tune=None, dlead=0, d_buf=None,
            d_offs=None, nbytes=None):
    """One device call: host arrays of every output (each with its guard entries; `out` with GUARD bytes of FILL on
    either side, its first byte dlead bytes past a 64-aligned address)."""
    n = offs.size - 1
    max_out = n if max_out is None else max_out
    cnt, ob = err_sizes(n, max_out, ipver, buf.size if nbytes is None else nbytes)
    t = dict(n_out=filled(cnt["n_out"], torch.int64), out_off=filled(cnt["out_off"], torch.int64),
             src_frame=filled(cnt["src_frame"], torch.int32), status=filled(cnt["status"], torch.uint8))
    out = torch.full((GUARD + dlead + ob + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    fn = nsx.icmp_err_ipv4_dev if ipver == 4 else nsx.icmp_err_ipv6_dev
    res = fn(d(buf) if d_buf is None else d_buf, d(offs) if d_offs is None else d_offs, d(np.asarray(req, np.uint32)),
             OUR[ipver] if src is None else src, arg=None if arg is None else d(np.asarray(arg, np.uint32)), ttl=ttl,
             ident0=ident0, max_out=max_out, out=dict(t, out=out[GUARD + dlead:]), tune=tune)
    assert all(res[k] is t[k] for k in t)
    got = {k: host(t[k]).view(_DT[k]) for k in t}
    a = host(out)
    assert (a[:dlead] == FILL).all()
    got["out"] = a[dlead:]
    return got


def err_want(buf, offs, req, arg, ipver, src=None, ttl=64, ident0=0, max_out=None, nbytes=None):
    """The model's outputs laid into FILL-filled arrays of err_gpu's sizes: (arrays, the model's dict)."""
    n = offs.size - 1
    max_out = n if max_out is None else max_out
    o = M.err(buf, offs, req, arg, OUR[ipver] if src is None else src, ttl, ident0, max_out, ipver)
    cnt, ob = err_sizes(n, max_out, ipver, np.asarray(buf).size if nbytes is None else nbytes)
    w = {}
    for k, c in cnt.items():
        a = np.full(max(c, 1) * np.dtype(_DT[k]).itemsize, FILL, np.uint8).view(_DT[k])
        v = np.asarray([o["n_out"]], np.uint64) if k == "n_out" else np.asarray(o[k]).reshape(-1)
        a[:v.size] = v
        w[k] = a
    assert o["out"].size <= ob, "the worst-case extent of the header comment does not hold"
    w["out"] = np.full(GUARD + ob + GUARD, FILL, np.uint8)
    w["out"][GUARD:GUARD + o["out"].size] = o["out"]
    return w, o


def err_same(got, w, o, what=""):
    for k in ("status", "n_out", "src_frame", "out_off", "out"):
        if not np.array_equal(got[k], w[k]):
            at = np.nonzero(got[k] != w[k])[0]
            extra = ""
            if k == "out":
                s = int(np.searchsorted(o["out_off"], at[0] - GUARD, side="right")) - 1
                extra = (f" (output byte {at[0] - GUARD}: message {s}, its byte "
                         f"{at[0] - GUARD - int(o['out_off'][max(s, 0)])})")
            raise AssertionError(f"{what} {k}: {at.size} entries differ, first at {at[0]}{extra}: got {got[k][at[:8]]}, "
                                 f"want {w[k][at[:8]]} (n_out got {got['n_out'][0]}, want {w['n_out'][0]})")


def err_check(buf, offs, req, arg, ipver, tunes=(None,), dleads=(0,), what="", **kw):
    """The device against the model over every tune and destination alignment given; returns the model's dict."""
    w, o = err_want(buf, offs, req, arg, ipver, **kw)
    for tune in tunes:
        for dlead in dleads:
            err_same(err_gpu(buf, offs, req, arg, ipver, tune=tune, dlead=dlead, **kw), w, o,
                     f"{what} tune={tune} dlead={dlead}")
    return o


# ------------------------------------------------------------------ receive verify
def rx_gpu(buf, offs, ipver, tune=None, d_buf=None, d_offs=None):
    """One device call: mask words (one guard word behind them), ip_raw (IPv4), icmp_raw and type with a guard entry."""
    n = offs.size - 1
    nw = (n + 63) // 64
    mask = filled(nw + 1, torch.int64)
    ipr, raw, typ = (filled(n + 1, torch.int16) for _ in range(3))
    kw = dict(ip_raw=ipr) if ipver == 4 else {}
    fn = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    got = fn(d(buf) if d_buf is None else d_buf, d(offs) if d_offs is None else d_offs, mask=mask, icmp_raw=raw,
             type=typ, tune=tune, **kw)
    assert got is mask
    u16 = lambda t: host(t).view(np.uint16)  # noqa: E731
    return dict(mask=host(mask).view(np.uint64), ip_raw=u16(ipr), icmp_raw=u16(raw), type=u16(typ))


def rx_want(buf, offs, ipver):
    n = offs.size - 1
    v = M.verify(buf, offs, ipver)
    fill16 = np.full(2, FILL, np.uint8).view(np.uint16)[0]
    w = dict(mask=np.concatenate([mask_words(v["ok"].astype(np.uint8)).reshape(-1),
                                  np.full(8, FILL, np.uint8).view(np.uint64)]))
    for k in ("ip_raw", "icmp_raw", "type"):
        w[k] = np.concatenate([v[k], [fill16]]).astype(np.uint16) if (k != "ip_raw" or ipver == 4) else \
            np.full(n + 1, fill16, np.uint16)
    assert w["mask"].size == (n + 63) // 64 + 1
    return w, v


def rx_check(buf, offs, ipver, tunes=(None,), what=""):
    w, v = rx_want(buf, offs, ipver)
    for tune in tunes:
        got = rx_gpu(buf, offs, ipver, tune=tune)
        for k in ("mask", "ip_raw", "icmp_raw", "type"):
            if not np.array_equal(got[k], w[k]):
                at = np.nonzero(got[k] != w[k])[0]
                raise AssertionError(f"{what} tune={tune} {k}: {at.size} entries differ, first at {at[0]}: got "
                                     f"{got[k][at[:8]]}, want {w[k][at[:8]]}")
    return v


# ------------------------------------------------------------------ echo reply
HIT_FILL = 0x5C


def echo_gpu(buf, offs, valid, ttl, ipver, d_valid=None):
    """One device call: (arena bytes with GUARD bytes of FILL on either side of buf, hit words incl. one guard word)."""
    n = offs.size - 1
    arena = torch.full((GUARD + buf.size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    view = arena[GUARD:GUARD + buf.size]
    view.copy_(dev(buf))
    hit = torch.full((8 * ((n + 63) // 64 + 1),), HIT_FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    fn = nsx.icmp_echo_reply_ipv4_dev if ipver == 4 else nsx.icmp_echo_reply_ipv6_dev
    res = fn(view, d(offs), d_words(valid) if d_valid is None else d_valid, ttl=ttl, hit=hit)
    assert res is hit
    return host(arena), host(hit).view(np.uint64)


def echo_want(buf, offs, valid, ttl, ipver):
    n = offs.size - 1
    out, hit = M.echo(buf, offs, valid, ttl, ipver)
    guard = np.full(GUARD, FILL, np.uint8)
    w = np.concatenate([mask_words(hit.astype(np.uint8)).reshape(-1), np.full(8, HIT_FILL, np.uint8).view(np.uint64)])
    assert w.size == (n + 63) // 64 + 1
    return np.concatenate([guard, out, guard]), w, hit


def echo_check(buf, offs, valid, ttl, ipver, what="", d_valid=None):
    """The whole arena and the hit words against the model; returns the model's hit booleans."""
    got, ghit = echo_gpu(buf, offs, valid, ttl, ipver, d_valid=d_valid)
    want, whit, hit = echo_want(buf, offs, valid, ttl, ipver)
    if not np.array_equal(ghit, whit):
        at = np.nonzero(ghit != whit)[0]
        raise AssertionError(f"{what}: hit word {at[0]}: got {ghit[at[0]]:#018x}, want {whit[at[0]]:#018x}")
    if not np.array_equal(got, want):
        at = np.nonzero(got != want)[0]
        b = int(at[0]) - GUARD
        i = int(np.searchsorted(offs, np.uint64(max(b, 0)), side="right")) - 1
        raise AssertionError(f"{what}: {at.size} bytes differ, first at buffer byte {b} (frame {i}, its byte "
                             f"{b - int(offs[max(i, 0)])}): got {got[at[:8]]}, want {want[at[:8]]}")
    return hit
