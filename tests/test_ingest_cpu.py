"""CPU: the parts of the micrograph ingest (spr_pick_amd/ingest.py) that need no GPU — the binned
geometry and the two coordinate maps, the command line (`joint eval --bin N`, `joint bin`), the fake-tensor shapes of
the two operators and the argument checking of the C entry points."""
import numpy as np
import pytest
import torch


def test_geometry_and_coordinate_round_trips():
    from spr_pick_amd import ingest
    for N in range(1, 17):
        for ny, nx in ((67, 131), (64, 64), (16, 33), (4096 + N - 1, 4096 + N // 2)):
            by, bx, oy, ox = ingest.binned_geometry(ny, nx, N)
            assert (by, bx) == (ny // N, nx // N) and (oy, ox) == ((ny % N) // 2, (nx % N) // 2)
            assert oy + by * N <= ny and ox + bx * N <= nx and ny - by * N < N and nx - bx * N < N
            # binned -> raw -> binned is the identity, and the raw point is the centre sample of the block
            xb, yb = np.meshgrid(np.arange(bx), np.arange(by))
            x, y = ingest.to_unbinned(xb, yb, N, ox, oy)
            assert x.min() == ox + N // 2 and x.max() == ox + N * (bx - 1) + N // 2 < nx and y.max() < ny
            xb2, yb2, inside = ingest.to_binned(x, y, N, ox, oy, bx, by)
            assert np.array_equal(xb2, xb) and np.array_equal(yb2, yb) and inside.all()
            # every raw sample: inside exactly the kept area, and inside its own block
            xs, ys = np.arange(nx), np.arange(ny)
            bxs, _, in_x = ingest.to_binned(xs, np.full(nx, oy), N, ox, oy, bx, by)
            _, bys, in_y = ingest.to_binned(np.full(ny, ox), ys, N, ox, oy, bx, by)
            assert np.array_equal(in_x, (xs >= ox) & (xs < ox + bx * N)) and in_x.sum() == bx * N
            assert np.array_equal(in_y, (ys >= oy) & (ys < oy + by * N)) and in_y.sum() == by * N
            assert np.array_equal(bxs[in_x], np.repeat(np.arange(bx), N))
            assert np.array_equal(bys[in_y], np.repeat(np.arange(by), N))
    assert ingest.to_binned(-1, 0, 4, 0, 0, 10, 10)[2] == False      # noqa: E712  (floor division: -1 -> block -1)
    for bad in (0, 17, -1, 2.0):
        with pytest.raises(ValueError):
            ingest.binned_geometry(64, 64, bad)
    with pytest.raises(ValueError):
        ingest.binned_geometry(3, 64, 4)


def test_command_line_accepts_bin():
    from spr_pick_amd import cli
    p = cli.build_parser()
    base = ["eval", "-m", "x.wt", "-d", "t.txt"]
    assert vars(p.parse_args(base))["bin"] is None
    for n in (1, 8, 16):
        assert vars(p.parse_args(base + ["--bin", str(n)]))["bin"] == n
    args = vars(p.parse_args(["bin", "--dataset", "raw", "--bin", "8", "--out", "d", "--labels", "c.txt"]))
    assert (args["command"], args["dataset"], args["bin"], args["out"], args["labels"]) == ("bin", "raw", 8, "d", "c.txt")
    assert vars(p.parse_args(["bin", "-d", "raw", "--bin", "2", "-o", "d"]))["labels"] is None
    for bad in ("0", "17", "-2", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--bin", bad])
        with pytest.raises(SystemExit):
            p.parse_args(["bin", "--dataset", "raw", "--bin", bad, "--out", "d"])
    with pytest.raises(SystemExit):
        p.parse_args(["bin", "--dataset", "raw", "--out", "d"])          # --bin is required there


def test_fake_shapes_of_the_ingest_operators():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from spr_pick_amd import torch_ops
    assert {"ingest_bin", "ingest_finish"} <= set(torch_ops.registered())
    with FakeTensorMode():
        raw = torch.empty(67 * 131 * 2, dtype=torch.uint8, device="cuda")
        binned, rng = torch.ops.sprk.ingest_bin(raw, 1, 67, 131, 4)
        assert tuple(binned.shape) == (16, 32) and binned.dtype == torch.float32 and tuple(rng.shape) == (2,)
        u8, net = torch.ops.sprk.ingest_finish(binned, rng, True, True)
        assert tuple(u8.shape) == (16, 32) and u8.dtype == torch.uint8
        assert tuple(net.shape) == (32, 32) and net.dtype == torch.float32
        b2 = torch.empty(70, 17, device="cuda")
        u8, net = torch.ops.sprk.ingest_finish(b2, rng, False, True)
        assert u8.numel() == 0 and tuple(net.shape) == (96, 96)
        u8, net = torch.ops.sprk.ingest_finish(b2, rng, True, False)
        assert tuple(u8.shape) == (70, 17) and net.numel() == 0
    assert torch_ops.net_size(4096, 4096) == 4096 and torch_ops.net_size(33, 35) == 64


def test_c_entry_points_check_their_arguments():
    from spr_pick_amd import _lib
    assert {"sprk_ingest_ws_bytes", "sprk_ingest_bin", "sprk_ingest_finish"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    A = 0x100000                                   # never dereferenced: every call below is refused before a launch
    assert L.sprk_ingest_ws_bytes(64, 64, 4) > 0
    assert L.sprk_ingest_ws_bytes(64, 64, 0) == 0 and L.sprk_ingest_ws_bytes(64, 64, 17) == 0
    assert L.sprk_ingest_ws_bytes(3, 64, 4) == 0
    assert L.sprk_ingest_bin(None, 1, 64, 64, 4, A, A, A, 256, None) == -1 and b"null" in L.sprk_last_error()
    assert L.sprk_ingest_bin(A, 12, 64, 64, 4, A, A, A, 256, None) == -1 and b"mode" in L.sprk_last_error()
    assert L.sprk_ingest_bin(A, 3, 64, 64, 4, A, A, A, 256, None) == -1 and b"mode" in L.sprk_last_error()
    for n in (0, 17):
        assert L.sprk_ingest_bin(A, 1, 64, 64, n, A, A, A, 256, None) == -1 and b"bin" in L.sprk_last_error()
    assert L.sprk_ingest_bin(A + 2, 1, 64, 64, 4, A, A, A, 256, None) == -1 and b"aligned" in L.sprk_last_error()
    assert L.sprk_ingest_bin(A, 1, 64, 64, 4, A, A, A, 8, None) == -2                      # SPRK_EWORKSPACE
    assert L.sprk_ingest_finish(None, 8, 8, A, A, A, 32, None) == -1 and b"null" in L.sprk_last_error()
    assert L.sprk_ingest_finish(A, 8, 8, A, None, None, 32, None) == -1 and b"null" in L.sprk_last_error()
    assert L.sprk_ingest_finish(A, 40, 8, A, None, A, 32, None) == -1 and b"network size" in L.sprk_last_error()
    assert L.sprk_ingest_finish(A, 8, 8, A, None, A, 40, None) == -1


def test_raw_reader_refuses_what_the_host_loader_refuses(tmp_path):
    """Header parsing needs no device: stacks, unknown modes and short files raise ValueError like load_image."""
    import struct
    from spr_pick_amd import ingest, micrograph_io
    p = str(tmp_path / "stack.mrc")
    with open(p, "wb") as f:
        micrograph_io.write_mrc(f, np.zeros((2, 8, 8), dtype=np.float32), extended_header=b"abc")
    with open(p, "rb") as f, pytest.raises(ValueError, match="single 2-D micrograph"):
        ingest.read_header(p, f)
    good = str(tmp_path / "one.mrc")
    with open(good, "wb") as f:
        micrograph_io.write_mrc(f, np.zeros((8, 9), dtype=np.float32), extended_header=b"abc")
    with open(good, "rb") as f:
        header, start = ingest.read_header(good, f)
    assert (header.ny, header.nx, header.mode, start) == (8, 9, 2, 1027)
    head = bytearray(open(good, "rb").read())
    struct.pack_into("<i", head, 12, 12)                                 # mode 12 (fp16) stays unsupported
    open(good, "wb").write(bytes(head))
    with open(good, "rb") as f, pytest.raises(ValueError, match="Unsupported MRC mode"):
        ingest.read_header(good, f)
    open(good, "wb").write(b"short")
    with open(good, "rb") as f, pytest.raises(ValueError):
        ingest.read_header(good, f)
