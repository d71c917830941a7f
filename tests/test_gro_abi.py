"""Receive coalescing's boundary (nsx_gro_*), on any host: the numpy restatement tests/_gro.py held to segmentation
offload's expansion (coalescing the frames of a super-segment batch gives the batch back), the symbols, every
NSX_EINVAL, validation before any device work, and the binding's extent checks. The GPU tests
(tests/test_gpu_gro.py) compare the kernels against tests/_gro.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nsx
import _gro
import _tso
import _tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CALLS = ("nsx_gro_ipv4_tcp_dev", "nsx_gro_ipv6_tcp_dev")
MSS_SET = _gro.MSS_SET
fake = ctypes.c_void_p(0x1000)
cut_batch, frames_of = _gro.cut_batch, _gro.frames_of


@pytest.mark.parametrize("opts", [False, True], ids=["noopt", "opts"])
@pytest.mark.parametrize("mss", MSS_SET)
@pytest.mark.parametrize("ipver", [4, 6])
def test_oracle_inverts_the_expansion(ipver, mss, opts):
    """Frames of a super-segment batch → tests/_gro.py → one super-segment per original one; tests/_tso.expected over
    that output reproduces the frames byte for byte, and the fields, mss, options and payload of every multi-frame
    super-segment equal the batch's own."""
    b = cut_batch(ipver, mss, opts, lead=1)
    s = b.sup
    buf, offs, valid = frames_of(b)
    out = _gro.gro(buf, offs, valid, ipver)
    assert out["n_super"] == b.n
    assert np.array_equal(out["frame_cnt"], np.diff(b.first)) and np.array_equal(out["first_frame"], b.first[:-1])
    assert np.array_equal(out["frame_seg"], b.seg)
    b2 = _gro.as_batch(out, ipver)
    assert np.array_equal(b2.first, _tso.count(b2.sup.data_off, b2.mss))  # frame_cnt is what the offload will cut
    buf2, _, c2 = _tso.expected(b2)
    body2, offs2 = _gro.dense(buf2, b2.off, c2.flen)
    assert np.array_equal(offs2, offs - offs[0])
    assert np.array_equal(body2, buf[int(offs[0]):int(offs[-1])])
    multi = np.nonzero(np.diff(b.first) > 1)[0]
    assert multi.size >= 8
    for i in multi:
        for k, v in s.fields.items():
            assert out[k][i] == v[i], (i, k)
        for k in ("src", "dst", "ttl"):
            assert np.array_equal(out[k][i], s.ip[k][i]), (i, k)
        if ipver == 4:
            assert out["ident"][i] == s.ip["ident"][i] and out["tclass"][i] == 0 and out["flow"][i] == 0
        else:
            assert out["ident"][i] == 0 and out["tclass"][i] == s.ip["tclass"][i]
            assert out["flow"][i] == s.ip["flow"][i] & 0xFFFFF
        assert out["mss"][i] == mss
        want_opts = b"" if s.opt_off is None else s.opts[int(s.opt_off[i]):int(s.opt_off[i + 1])].tobytes()
        assert out["opts"][int(out["opt_off"][i]):int(out["opt_off"][i + 1])].tobytes() == want_opts
        assert np.array_equal(out["data"][int(out["data_off"][i]):int(out["data_off"][i + 1])],
                              s.data[int(s.data_off[i]):int(s.data_off[i + 1])])


def test_oracle_window_rule_and_breaks():
    """The worked examples of the header: a strictly decreasing chain, a chain with two equal short tails, a
    non-member in the middle of a run, a cleared mask bit."""
    rng = np.random.default_rng(0x6A0)

    def chain(pays, ipver=4):
        return _gro.pack(_gro.case_frames(_gro.flow_case(rng, ipver, pays)))

    buf, offs = chain([1000, 800, 600, 400, 200])
    out = _gro.gro(buf, offs, np.ones(5, bool), 4)
    assert out["frame_cnt"].tolist() == [2, 1, 1, 1] and out["mss"].tolist() == [1000, 600, 400, 200]
    buf, offs = chain([1000, 1000, 500, 500])
    out = _gro.gro(buf, offs, np.ones(4, bool), 4)
    assert out["frame_cnt"].tolist() == [3, 1] and out["frame_seg"].tolist() == [0, 0, 0, 1]
    buf, offs = chain([700] * 6, ipver=6)
    out = _gro.gro(buf, offs, np.ones(6, bool), 6)
    assert out["frame_cnt"].tolist() == [6] and int(out["data_off"][1]) == 4200
    valid = np.ones(6, bool)
    valid[2] = False
    out = _gro.gro(buf, offs, valid, 6)
    assert out["frame_cnt"].tolist() == [2, 3] and out["frame_seg"].tolist() == [0, 0, _gro.NONE, 1, 1, 1]
    assert _gro.gro(buf, offs, _mask_words(valid), 6)["frame_seg"].tolist() == out["frame_seg"].tolist()


def _mask_words(valid):
    pad = np.zeros((valid.size + 63) // 64 * 64, np.uint8)
    pad[:valid.size] = valid
    return np.packbits(pad, bitorder="little").view(np.uint64)


# ---------------------------------------------------------------- symbols
def test_gro_symbols_are_declared_and_exported(tmp_path):
    """nsx_csum.h declares nsx_gro_work_bytes and the two device calls, the new nsx_gro_tune.h their _tuned twins
    (nsx_tune.h only includes it); the library exports all five; the header states the scope; and a plain C caller
    compiles against them and gets the documented codes from the validation."""
    inc = os.path.join(ROOT, "include")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)  # noqa: E731
    text = open(os.path.join(inc, "nsx_csum.h")).read()
    plain = set(re.findall(r"^int (nsx_gro_[a-z_0-9]+)\(", strip(text), flags=re.M))
    tuned = set(re.findall(r"^int (nsx_gro_[a-z_0-9]+)\(", strip(open(os.path.join(inc, "nsx_gro_tune.h")).read()),
                           flags=re.M))
    assert plain == set(DEV_CALLS) | {"nsx_gro_work_bytes"}
    assert tuned == {f + "_tuned" for f in DEV_CALLS}
    tune_h = strip(open(os.path.join(inc, "nsx_tune.h")).read())
    assert '#include "nsx_gro_tune.h"' in tune_h and "nsx_gro_" not in tune_h.replace("nsx_gro_tune.h", "")
    out = subprocess.run(["nm", "-D", "--defined-only", nsx.LIB_PATH], capture_output=True, text=True).stdout
    assert plain | tuned <= set(re.findall(r" T (nsx_\w+)", out))
    assert nsx.abi_version() == 2
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for word in ("by adjacency only", "no flow table", "three-frame window", "no 64 KiB cap", "no _host forms",
                 "its options dropped"):
        assert word in flat, word
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include "nsx_tune.h"
int main(void) {
    nsx_gro_out o = {0};
    nsx_tune t = {0};
    uint64_t need = 0, offs[1] = {0}, mask[1] = {0};
    if (nsx_gro_work_bytes(1000, &need) != NSX_OK || need < 16 * 1000) return 1;
    if (nsx_gro_work_bytes(0xFFFFFFFFull, &need) != NSX_EINVAL || nsx_gro_work_bytes(1, 0) != NSX_EINVAL) return 2;
    if (nsx_gro_ipv4_tcp_dev(offs, offs, 0, mask, &o, offs, 64, 0) != NSX_EINVAL) return 3;
    if (nsx_gro_ipv6_tcp_dev_tuned(offs, offs, 0, mask, 0, offs, 64, 0, &t) != NSX_EINVAL) return 4;
    return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(nsx.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", inc, "-L", libdir, "-lnsx_csum",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- validation
def _out(null=()):
    return nsx.GroOut(*[None if k in null else 0x1000 for k, _, _ in nsx.GRO_FIELDS])


def _call(name, n=100, tuned=False, out=None, **kw):
    a = dict(base=fake, offsets=fake, valid=fake, work=fake, work_bytes=nsx.gro_work_bytes(min(n, 1 << 20)))
    a.update(kw)
    o = _out() if out is None else out
    args = [a["base"], a["offsets"], n, a["valid"], None if o == "null" else ctypes.byref(o), a["work"], a["work_bytes"],
            None]
    if tuned:
        return getattr(nsx.lib(), name + "_tuned")(*args, ctypes.byref(nsx.Tune(run_segs=64)))
    return getattr(nsx.lib(), name)(*args)


def test_gro_device_calls_validate_before_any_device_work():
    """NULL pointers, every NULL member of nsx_gro_out, n >= 2^32 - 1 and a workspace one byte short are NSX_EINVAL
    before anything else; a well-formed call on a host with no GPU is then NSX_ENODEV, n == 0 included (it has
    stream work to do: n_super and the leading offsets)."""
    E = nsx.NSX_EINVAL
    for name in DEV_CALLS:
        for tuned in (False, True):
            for kw in (dict(base=None), dict(offsets=None), dict(valid=None), dict(work=None), dict(out="null"),
                       dict(n=0xFFFFFFFF, work_bytes=1 << 62), dict(n=1 << 32, work_bytes=1 << 62),
                       dict(work_bytes=nsx.gro_work_bytes(100) - 1), dict(work_bytes=0),
                       dict(n=0, work_bytes=nsx.gro_work_bytes(0) - 1), dict(n=0, offsets=None)):
                assert _call(name, tuned=tuned, **kw) == E, kw
            for k, _, _ in nsx.GRO_FIELDS:
                assert _call(name, tuned=tuned, out=_out(null=(k,))) == E, k
            if nsx.device_count() == 0:
                assert _call(name, tuned=tuned) == nsx.NSX_ENODEV
                assert _call(name, tuned=tuned, n=0, base=None, valid=None) == nsx.NSX_ENODEV
                assert _call(name, tuned=tuned, n=0xFFFFFFFE, work_bytes=1 << 62) == nsx.NSX_ENODEV


def test_gro_work_bytes():
    """Grows with n, covers the per-frame scratch (16 bytes a frame and the block sums of the smallest scan block),
    and refuses n >= 2^32 - 1."""
    w = [nsx.gro_work_bytes(n) for n in (0, 1, 63, 64, 4096, 4097, 1 << 20)]
    assert all(b > a for a, b in zip(w, w[1:])) and w[0] >= 8
    assert 16 << 20 <= w[-1] <= 20 << 20
    with pytest.raises(nsx.NsxError) as e:
        nsx.gro_work_bytes(0xFFFFFFFF)
    assert e.value.code == nsx.NSX_EINVAL
    assert nsx.gro_work_bytes(0xFFFFFFFE) > 16 * 0xFFFFFFFE


def test_gro_binding_checks_extents_before_the_c_call():
    """Every given tensor is checked before the C call (CPU tensors here: a well-formed call is then refused as not
    on a device): a short mask, each short output, a short workspace, wrong element sizes, unknown names."""
    import torch
    n = 70
    offs = torch.arange(n + 1, dtype=torch.int64) * 60
    buf = torch.zeros(60 * n, dtype=torch.uint8)
    valid = torch.zeros(2, dtype=torch.int64)
    for ipver, fn in ((4, nsx.gro_ipv4_tcp_dev), (6, nsx.gro_ipv6_tcp_dev)):
        alen = 4 if ipver == 4 else 16
        cases = [(dict(valid=valid[:1]), " valid"), (dict(valid=None), "`valid` is required"),
                 (dict(valid=torch.zeros(4, dtype=torch.int32)), "8-byte elements"),
                 (dict(offsets=torch.zeros(n + 1, dtype=torch.int32)), "8-byte elements"),
                 (dict(work=torch.zeros(nsx.gro_work_bytes(n) - 1, dtype=torch.uint8)), " work"),
                 (dict(out={"bogus": buf}), "unknown output"),
                 (dict(out={"src": torch.zeros(alen * n - 1, dtype=torch.uint8)}), " src"),
                 (dict(out={"n_super": torch.zeros(1, dtype=torch.int32)}), "8-byte elements")]
        for k, dt, count in nsx.GRO_FIELDS:
            need = count(n, alen, buf.numel())
            if need > 1:
                cases.append((dict(out={k: torch.zeros(need - 1, dtype=getattr(torch, dt))}), f" {k}:"))
        cases.append((dict(), "device"))
        for kw, msg in cases:
            args = dict(buf=buf, offsets=offs, valid=valid)
            args.update(kw)
            with pytest.raises(ValueError) as e:
                fn(**args)
            assert msg in str(e.value), (msg, str(e.value))
