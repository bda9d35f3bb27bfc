"""GPU: TIFF movies in (csrc/tiff.hip, ``torch.ops.sprk.tiff_decode``, spr_pick_amd/tiffio.py): the kernel bit
for bit against the model of its contract (tests/tiff_model.py) in ``out`` and ``status``, with 4 KiB guard bands of a
sentinel before and after ``out``, on the smallest inputs that reach each branch; the refusals of the C ABI; and ``joint
align`` end to end, which must write from an LZW TIFF the bytes it writes from the MRC of the same values."""
import ctypes
import os

import numpy as np
import pytest
import torch

import align_model
import tiff_model
from extract_model import write_raw_mrc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, 0xA5


def pack(pieces, lead=1, gap=0):
    """encoded strips laid back to back after ``lead`` bytes -> (src bytes, offsets, lengths)"""
    src, offs, lens = bytearray(b"\xEE" * lead), [], []
    for p in pieces:
        offs.append(len(src))
        lens.append(len(p))
        src += p + b"\xEE" * gap
    return bytes(src), offs, lens


def device_decode(src, offs, lens, outs, compression=5, widen=False, out_elems=None):
    """one launch through the operator, between guard bands -> (out as the model returns it, status); asserts the bands and
    whatever of ``out`` lies past the strips' sum still hold the sentinel"""
    from spr_pick_amd import torch_ops  # noqa: F401  (registers torch.ops.sprk)
    total = sum(min(max(int(v), 0), 1 << 40) for v in outs)
    cap = total if out_elems is None else out_elems
    item = 2 if widen else 1
    buf = torch.full((2 * GUARD + cap * item + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + cap * item]
    status = torch.full((len(offs),), -1, dtype=torch.int32, device="cuda")
    dev = [torch.tensor(list(v), dtype=torch.int64, device="cuda") for v in (offs, lens, outs)]
    s = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    assert torch.ops.sprk.tiff_decode(s, dev[0], dev[1], dev[2], compression, widen, out, status) is None
    whole = buf.cpu().numpy()
    assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + cap * item:] == SENTINEL).all(), "a guard band was written"
    written = min(total, cap) * item
    assert (whole[GUARD + written:GUARD + cap * item] == SENTINEL).all(), "out was written past the strips' sum"
    assert torch.equal(s.cpu(), torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()))
    got = whole[GUARD:GUARD + cap * item].copy()
    return (got.view("<u2") if widen else got), status.cpu().numpy(), min(total, cap)


def check(src, offs, lens, outs, compression=5, widen=False, out_elems=None, want_status=None):
    want, want_st = tiff_model.decode(src, offs, lens, outs, compression, widen, out_elems)
    got, st, written = device_decode(src, offs, lens, outs, compression, widen, out_elems)
    differ = int((got[:written] != want[:written]).sum())
    print("%d strip(s), %d -> %d bytes: statuses %s, %d bytes differ from the model"
          % (len(offs), sum(max(int(v), 0) for v in lens), written, sorted(set(st.tolist())), differ))
    assert np.array_equal(st, want_st), (st.tolist()[:20], want_st.tolist()[:20])
    assert differ == 0
    if want_status is not None:
        assert st.tolist() == list(want_status)
    return got, st


def poisson_frame(ny=37, nx=96, dtype="u1", seed=5):
    return np.random.RandomState(seed).poisson(1.0, size=(ny, nx)).astype(dtype)


def strips_of(frame, rows, encode=tiff_model.lzw_encode):
    raws = [frame[r:r + rows].tobytes() for r in range(0, frame.shape[0], rows)]
    return [encode(r) for r in raws], [len(r) for r in raws], raws


# ---- the kernel against the model ------------------------------------------------------------------------------------------
def test_random_bytes_pass_every_width_and_a_clear_mid_strip():
    data = np.random.RandomState(3).randint(0, 256, size=12000).astype(np.uint8).tobytes()
    src, offs, lens = pack([tiff_model.lzw_encode(data)])
    got, _ = check(src, offs, lens, [len(data)], want_status=[0])
    assert got.tobytes() == data


@pytest.mark.parametrize("period", [1, 2, 3])
def test_long_strings_of_a_repeated_pattern(period):
    """the "code == next free" case at every step, and strings of several hundred bytes: the wave-wide copy in passes"""
    data = (bytes([7, 200, 31][:period]) * 40000)[:60001]
    src, offs, lens = pack([tiff_model.lzw_encode(data)], lead=3)
    got, _ = check(src, offs, lens, [len(data)], want_status=[0])
    assert got.tobytes() == data


def test_a_full_table_that_is_never_cleared_reaches_far_back():
    """a writer that sends no Clear: the table fills and stays, and the strings of its entries lie further back in the
    output than any window of recent bytes a decoder may keep"""
    data = np.random.RandomState(15).poisson(1.0, size=150000).astype(np.uint8).tobytes()
    enc = tiff_model.lzw_encode(data, table_limit=1 << 30)
    assert sum(1 for c, _ in codes_of(enc) if c == 256) == 1
    src, offs, lens = pack([enc])
    got, _ = check(src, offs, lens, [len(data)], want_status=[0])
    assert got.tobytes() == data


@pytest.mark.parametrize("rows", [1, 8, 37])
@pytest.mark.parametrize("lead", [1, 2, 3])
def test_poisson_counts_in_strips_at_odd_offsets(rows, lead):
    frame = poisson_frame()
    enc, outs, _ = strips_of(frame, rows)
    src, offs, lens = pack(enc, lead=lead)
    assert any(o % 4 for o in offs) and (lead == 2 or any(o % 2 for o in offs)) and outs[-1] == (37 - rows * ((37 - 1) // rows)) * 96
    got, _ = check(src, offs, lens, outs, want_status=[0] * len(offs))
    assert got.tobytes() == frame.tobytes()


@pytest.mark.parametrize("dtype", ["<u2", "<i2", "<f4"])
def test_samples_of_several_bytes(dtype):
    """strings cross sample boundaries: the decoder knows bytes only"""
    rng = np.random.RandomState(8)
    frame = rng.poisson(1.0, size=(37, 96)).astype(dtype) if dtype != "<f4" else \
        (rng.poisson(1.0, size=(37, 96)) * 0.37 + rng.randint(0, 2, size=(37, 96)) * 1e-3).astype("<f4")
    enc, outs, _ = strips_of(frame, 8)
    src, offs, lens = pack(enc)
    got, _ = check(src, offs, lens, outs, want_status=[0] * len(offs))
    assert got.tobytes() == frame.tobytes()


def test_uint8_widened_to_uint16():
    frame = poisson_frame(seed=9)
    frame[0, :4] = [255, 128, 0, 1]
    enc, outs, _ = strips_of(frame, 8)
    src, offs, lens = pack(enc)
    got, _ = check(src, offs, lens, outs, widen=True, want_status=[0] * len(offs))
    assert got.dtype == np.dtype("<u2") and np.array_equal(got.reshape(37, 96), frame.astype(np.uint16))


@pytest.mark.parametrize("widen", [False, True])
def test_stored_strips(widen):
    frame = poisson_frame(seed=10)
    _, outs, raws = strips_of(frame, 8)
    src, offs, lens = pack(raws, lead=3, gap=5)
    got, _ = check(src, offs, lens, outs, compression=1, widen=widen, want_status=[0] * len(offs))
    assert np.array_equal(got.reshape(37, 96), frame)
    # a stored strip shorter than its rows: what is there, zeros after it, status 2; a longer one: its head
    lens2 = list(lens)
    lens2[1], lens2[2] = 100, lens[2] + 4
    got, st = check(src, offs, lens2, outs, compression=1, widen=widen)
    assert st.tolist() == [0, 2, 0, 0, 0] and not got[outs[0] + 100:outs[0] + outs[1]].any()


def test_a_stream_without_eoi_and_one_with_bytes_after_it():
    frame = poisson_frame(seed=11)
    enc, outs, _ = strips_of(frame, 8, lambda r: tiff_model.lzw_encode(r, eoi=False))
    src, offs, lens = pack(enc)
    got, _ = check(src, offs, lens, outs, want_status=[0] * len(offs))
    assert got.tobytes() == frame.tobytes()
    enc, outs, _ = strips_of(frame, 8, lambda r: tiff_model.lzw_encode(r) + b"\xFF\x00\xFF\x80" * 3)
    src, offs, lens = pack(enc)
    got, _ = check(src, offs, lens, outs, want_status=[0] * len(offs))
    assert got.tobytes() == frame.tobytes()
    enc, outs, _ = strips_of(frame, 8, lambda r: tiff_model.lzw_encode(r, clear_every=50))     # Clears early
    src, offs, lens = pack(enc)
    got, _ = check(src, offs, lens, outs, want_status=[0] * len(offs))
    assert got.tobytes() == frame.tobytes()


def codes_of(enc):
    """the (code, width) list of a valid stream"""
    codes, bitpos, nxt, prev = [], 0, 258, False
    while True:
        w = tiff_model.width_of(nxt)
        code = tiff_model.read_code(enc, bitpos, w)
        bitpos += w
        codes.append((code, w))
        if code == 257:
            return codes
        if code == 256:
            nxt, prev = 258, False
        else:
            nxt, prev = nxt + (1 if prev and nxt < 4096 else 0), True


def repack(codes):
    w = tiff_model.BitWriter()
    for code, width in codes:
        w.put(code, width)
    return w.done()


def test_malformed_streams_give_the_models_status_and_bytes():
    """Inputs the contract defines an answer for: the first error of a strip is its status, the bytes before it stay, zeros
    follow, and the strips beside it decode as if it were sound."""
    frame = poisson_frame(seed=12)
    enc, outs, raws = strips_of(frame, 8)
    rng = np.random.RandomState(13)
    # strip 1: the input ends early; strip 2: a code above the next free one at code 40; strip 3: 2 KB of random bytes
    bad = list(enc)
    bad[1] = enc[1][:len(enc[1]) // 2]
    codes = codes_of(enc[2])
    nxt = 258 + 39                                               # the decoder's next free code when it reads code 40 (after the Clear)
    codes[41] = (nxt + 5, codes[41][1])
    bad[2] = repack(codes)
    bad[3] = rng.randint(0, 256, size=2048).astype(np.uint8).tobytes()
    src, offs, lens = pack(bad)
    got, st = check(src, offs, lens, outs)
    assert st[0] == 0 and st[1] == 2 and st[2] == 1 and st[3] in (1, 2, 3) and st[4] == 0
    assert got[:outs[0]].tobytes() == raws[0] and got[sum(outs[:4]):].tobytes() == raws[4]
    ok = tiff_model.lzw_decode(bad[2], outs[2])[0]
    assert ok[:30] == raws[2][:30] and not any(ok[-100:])                     # what came before the bad code stays
    # a valid stream asked for fewer bytes than it decodes to: cut at the strip's end, status 3 (or 0 at a string's end)
    src, offs, lens = pack(enc)
    short = [o - 7 for o in outs]
    got, st = check(src, offs, lens, short)
    assert set(st.tolist()) <= {0, 3} and 3 in st.tolist()
    longer = [o + 3 for o in outs]                               # and for more: EOI comes first, status 2, zeros at the end
    got, st = check(src, offs, lens, longer, want_status=[2] * len(offs))
    # tables that point past the bytes, before them, or nowhere: clamped, never followed
    n = len(src)
    wild_off = [offs[0], n - 10, n + 5, -20, 2 ** 62, offs[4]]
    wild_len = [lens[0], 1000, 50, 40, 2 ** 62, -1]
    check(src, wild_off, wild_len, outs + [50])
    # outputs that do not fit ``out``, and sizes that are no sizes
    check(src, offs, lens, outs, out_elems=sum(outs) - 1000)
    check(src, offs, lens, [outs[0], -5, 2 ** 40, outs[3], outs[4]], out_elems=sum(outs))
    check(src, offs, lens, outs, out_elems=sum(outs) + 333)


def test_600_strips_in_one_launch():
    """workgroups of several waves, and more strips than a handful of compute units hold at once; a few are damaged"""
    rng = np.random.RandomState(14)
    pieces, outs = [], []
    for s in range(600):
        n = int(rng.randint(1, 400))
        kind = s % 4
        raw = (rng.poisson(1.0, size=n) if kind < 2 else rng.randint(0, 256, size=n) if kind == 2
               else np.full(n, s & 255)).astype(np.uint8).tobytes()
        e = tiff_model.lzw_encode(raw, eoi=(s % 5 != 0))
        if s % 97 == 0:
            e = e[:len(e) // 2]
        pieces.append(e)
        outs.append(n)
    src, offs, lens = pack(pieces)
    _, st = check(src, offs, lens, outs)
    assert (st != 0).sum() >= 3 and (st == 0).sum() >= 580


def test_refusals_launch_nothing():
    from spr_pick_amd import _lib
    L = _lib.lib()
    frame = poisson_frame()
    enc, outs, _ = strips_of(frame, 8)
    src, offs, lens = pack(enc)
    s = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    t = [torch.tensor(v, dtype=torch.int64, device="cuda") for v in (offs, lens, outs)]
    out = torch.full((sum(outs),), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(offs),), -1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(src=s.data_ptr(), nbytes=len(src), off=t[0].data_ptr(), len=t[1].data_ptr(), so=t[2].data_ptr(), n=len(offs),
                comp=5, widen=0, out=out.data_ptr(), cap=sum(outs), status=status.data_ptr())

    def call(**change):
        a = dict(good, **change)
        return L.sprk_tiff_decode(a["src"], a["nbytes"], a["off"], a["len"], a["so"], a["n"], a["comp"], a["widen"], a["out"],
                                  a["cap"], a["status"], stream)

    torch.cuda.synchronize()
    before = L.sprk_launch_count()
    cases = [(dict(src=None), b"null"), (dict(out=None), b"null"), (dict(status=None), b"null"), (dict(off=None), b"null"),
             (dict(nbytes=0), b"bytes of strips"), (dict(n=0), b"strips"), (dict(n=(1 << 20) + 1), b"strips"),
             (dict(comp=8), b"compression"), (dict(comp=0), b"compression"), (dict(widen=2), b"widen"),
             (dict(cap=0), b"decoded bytes"), (dict(src=s.data_ptr() + 1), b"aligned"), (dict(out=out.data_ptr() + 2), b"aligned"),
             (dict(off=t[0].data_ptr() + 4), b"aligned"), (dict(status=status.data_ptr() + 2), b"aligned"),
             (dict(out=s.data_ptr()), b"out must not be src")]
    for change, word in cases:
        assert call(**change) == -1, (change, L.sprk_last_error())
        assert L.sprk_last_error().startswith(b"tiff_decode: ") and word in L.sprk_last_error(), (change, L.sprk_last_error())
    torch.cuda.synchronize()
    assert L.sprk_launch_count() == before
    assert bool((out == SENTINEL).all()) and bool((status == -1).all())
    assert call() == 0, L.sprk_last_error()
    assert L.sprk_launch_count() == before + 1                                # one launch per frame
    assert out.cpu().numpy().tobytes() == frame.tobytes() and not bool(status.any())
    with pytest.raises(_lib.SprkError, match="int64"):
        torch.ops.sprk.tiff_decode(s, t[0].int(), t[1], t[2], 5, False, out, status)
    with pytest.raises(_lib.SprkError, match="contiguous"):
        torch.ops.sprk.tiff_decode(s, t[0], t[1], t[2], 5, False, torch.empty(2 * sum(outs), dtype=torch.uint8, device="cuda")[::2],
                                   status)


# ---- end to end --------------------------------------------------------------------------------------------------------------
NY, NX, FRAMES, ROWS = 128, 192, 8, 8
# sample type -> (the TIFF's, the MRC's, signal, offset of align_model.make_movie)
E2E = {"int8": ("i1", "i1", 8.0, 0.0), "int16": ("<i2", "<i2", 60.0, 900.0), "uint16": ("<u2", "<u2", 60.0, 900.0),
       "float32": ("<f4", "<f4", 60.0, 900.0), "uint8": ("u1", "<u2", 8.0, 100.0)}


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def make_pair(root, kind, seed=1):
    """root/mrc/mov.mrc and root/tif/mov.tiff of the same planted-drift movie -> (movie, drift)"""
    tif_t, mrc_t, signal, offset = E2E[kind]
    movie, _, drift = align_model.make_movie(NY, NX, FRAMES, seed, 1.0, signal=signal, offset=offset, dtype=np.float64)
    movie = movie.astype(tif_t)
    for d in ("mrc", "tif"):
        os.makedirs(os.path.join(root, d))
    write_raw_mrc(os.path.join(root, "mrc", "mov.mrc"), movie.astype(mrc_t))
    tiff_model.write_tiff(os.path.join(root, "tif", "mov.tiff"), movie, ROWS, big=(kind == "int16"))
    return movie, drift


def same_outputs(a, b, names=("mov.mrc", "mov_shifts.txt")):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in names:
        assert read_bytes(os.path.join(a, name)) == read_bytes(os.path.join(b, name)), name


@pytest.mark.parametrize("kind", list(E2E))
def test_joint_align_writes_the_same_bytes_from_tiff_and_mrc(kind, tmp_path):
    from spr_pick_amd import cli
    root = str(tmp_path)
    movie, drift = make_pair(root, kind)
    want = cli.start(["align", "--movies", os.path.join(root, "mrc"), "--out", os.path.join(root, "want")])
    got = cli.start(["align", "--movies", os.path.join(root, "tif"), "--out", os.path.join(root, "got")])
    same_outputs(os.path.join(root, "got"), os.path.join(root, "want"))
    assert got == want and got["mov"]["frames"] == FRAMES and got["mov"]["shape"] == [NY, NX]
    shifts = np.array(got["mov"]["shifts"])
    print("%s: worst |estimated - planted| %.3f raw pixels" % (kind, float(np.abs(shifts - drift).max())))
    assert float(np.abs(shifts).max()) > 1.0                                  # the frames were read, and they moved


def test_the_same_bytes_with_dose_weighting_and_with_references(tmp_path):
    from spr_pick_amd import cli
    root = str(tmp_path)
    make_pair(root, "int16")
    rng = np.random.RandomState(3)
    gain, dark = os.path.join(root, "gain.mrc"), os.path.join(root, "dark.mrc")
    write_raw_mrc(gain, rng.uniform(0.9, 1.1, size=(NY, NX)).astype(np.float32))
    write_raw_mrc(dark, rng.randint(0, 20, size=(NY, NX)).astype(np.int16))
    for tag, flags, names in (("dose", ["--dose", "1.0", "--apix", "1.5"], ("mov.mrc", "mov_shifts.txt", "mov_DW.mrc")),
                              ("refs", ["--gain", gain, "--dark", dark, "--hot_sigma", "6"],
                               ("mov.mrc", "mov_shifts.txt", "mov_defects.mrc"))):
        outs = []
        for d in ("mrc", "tif"):
            outs.append(os.path.join(root, tag + "_" + d))
            cli.start(["align", "--movies", os.path.join(root, d), "--out", outs[-1]] + flags)
        same_outputs(outs[1], outs[0], names)


def test_a_table_of_both_kinds_and_a_movie_that_does_not_stay_on_the_device(tmp_path):
    from spr_pick_amd import align, cli, micrograph_io
    root = str(tmp_path)
    make_pair(root, "uint16")
    os.rename(os.path.join(root, "tif", "mov.tiff"), os.path.join(root, "tif", "mov.tif"))
    table = os.path.join(root, "movies.txt")
    with open(table, "w") as f:
        f.write("image_name\tpath\na\t%s\nb\t%s\n" % (os.path.join(root, "mrc", "mov.mrc"), os.path.join(root, "tif", "mov.tif")))
    res = cli.start(["align", "--movies", table, "--out", os.path.join(root, "out")])
    assert res["a"] == res["b"]
    for ext in (".mrc", "_shifts.txt"):
        assert read_bytes(os.path.join(root, "out", "a" + ext)) == read_bytes(os.path.join(root, "out", "b" + ext))
    # frames decoded again for the second pass (residency counts decoded bytes): the same sum
    with align.open_movie(os.path.join(root, "tif", "mov.tif")) as m:
        assert isinstance(m, align.TiffMovie) and m.resident and m.frame_bytes == NY * NX * 2 and m.header.mode == 6
    total, drift, _, _ = align.align_movie(os.path.join(root, "tif", "mov.tif"), resident_bytes=FRAMES * NY * NX * 2 - 1)
    want, _, _ = micrograph_io.parse_mrc(read_bytes(os.path.join(root, "out", "b.mrc")))
    assert np.array_equal(total.cpu().numpy(), want)


def test_a_corrupt_strip_is_reported_and_no_sum_is_written(tmp_path):
    from spr_pick_amd import cli
    root = str(tmp_path)
    path = os.path.join(root, "tif", "mov.tiff")
    os.makedirs(os.path.join(root, "tif"))
    movie, _, _ = align_model.make_movie(NY, NX, FRAMES, 2, 1.0)
    tables = tiff_model.write_tiff(path, movie, ROWS)
    with open(path, "r+b") as f:
        f.seek(tables[3][5][0])
        f.write(b"\xFF\xFF")                                                  # the first code is 511: no literal
    with pytest.raises(ValueError, match=r"mov\.tiff: frame 3, strip 5: the LZW stream holds a code that is not in the table"):
        cli.start(["align", "--movies", os.path.join(root, "tif"), "--out", os.path.join(root, "out")])
    assert not os.path.exists(os.path.join(root, "out", "mov.mrc"))
