"""The in-process communicator of the band frame (NativeComm.local: csrc/comm.cpp LocalComm, csrc/halo.hip
copy_segments) alone, away from the sizes the band frame gives it at the benchmark shapes.

At 1920 x 1080 and 3840 x 2160 every AO row is a multiple of 16 bytes at a 16-byte offset, so every transfer of
tests/test_gpu_band_native.py takes copy_segments' 16-byte lanes, no list exceeds 16 segments and every rank sends
something.  Here: 1, 15, 16, 17 and 4097 bytes at byte offsets 0, 1 and 3 from an aligned base between 2 and 3 ranks,
one transfer past the 4096-block grid on each of the two paths, an all-gather of 17 ranks (17 segments: two launches),
and a zero-byte send beside others.  Every destination lies between sentinel bytes and is compared bytewise.

tests/test_band_odd.py holds the CPU half of the band frame's odd cases (helpers.BAND_ODD_CASES)."""
import threading

import pytest

from helpers import SENTINEL

pytestmark = pytest.mark.gpu

JOIN_S = 90   # a rank thread that has not finished by then is reported, not waited for


def _rank_threads(world, run):
    """run(k) on one host thread per rank; the first traceback of a rank fails the test."""
    errors = []

    def guarded(k):
        try:
            run(k)
        except Exception:  # noqa: BLE001 -- reported by the main thread
            import traceback
            errors.append((k, traceback.format_exc()))

    threads = [threading.Thread(target=guarded, args=(k,)) for k in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=JOIN_S)
    assert not any(t.is_alive() for t in threads), "a rank thread did not finish"
    assert not errors, errors


# ---- the communicator alone

def _payload(torch, n, seed):
    """n bytes that depend on every index and on the seed (never a constant run)."""
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    return ((i * 131 + (i >> 8) * 7 + 29 * seed + 1) % 251).to(torch.uint8)


class _Guarded:
    """n bytes at byte offset `off` from a 256-byte-aligned base, sentinel bytes all around."""

    def __init__(self, torch, n, off):
        self.torch, self.n, self.off = torch, n, off
        self.raw = torch.full((256 + off + n + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.view = self.raw[256 + off:256 + off + n]

    def check(self, want, what):
        assert self.torch.equal(self.view, want), f"{what}: payload"
        lo, hi = 256 + self.off, 256 + self.off + self.n
        assert bool((self.raw[:lo] == SENTINEL).all()) and bool((self.raw[hi:] == SENTINEL).all()), \
            f"{what}: a store outside the destination"


def _comm_threads(torch, world, body):
    """body(k, comm) on a stream and a host thread per rank of an in-process communicator."""
    from rsd.shard import NativeComm, NativeHub
    hub = NativeHub(world)
    comms = [NativeComm.local(hub, k) for k in range(world)]
    streams = [torch.cuda.Stream() for _ in range(world)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()

    def run(k):
        with torch.cuda.stream(streams[k]):
            body(k, comms[k])

    try:
        _rank_threads(world, run)
        torch.cuda.synchronize()
    finally:
        for c in comms:
            c.close()
        hub.close()


COMM_SIZES = (1, 15, 16, 17, 4097)
COMM_OFFSETS = (0, 1, 3)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [2, 3])
def test_comm_sizes_and_alignments(world):
    """NativeComm.all_gather and .exchange of 1, 15, 16, 17 and 4097 bytes at offsets 0, 1 and 3 from an aligned base:
    copy_segments takes its 16-byte lanes only where source, destination and size allow it, and a tail of a size that
    is no multiple of 16 arrives; bytewise, with sentinels around every destination.  One more exchange has an aligned
    source and a destination at offset 3."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    combos = [(n, off, off) for n in COMM_SIZES for off in COMM_OFFSETS] + [(16, 0, 3), (4096, 3, 0)]
    bufs = {}
    for ci, (n, so, do) in enumerate(combos):
        for k in range(world):
            src = _Guarded(torch, n, so)
            src.view.copy_(_payload(torch, n, 10 * ci + k))
            xs = {p: _Guarded(torch, n, so) for p in range(world) if p != k}
            for p, g in xs.items():
                g.view.copy_(_payload(torch, n, 1000 + 100 * ci + 10 * k + p))
            bufs[ci, k] = (src, _Guarded(torch, world * n, do), xs,
                           {p: _Guarded(torch, n, do) for p in range(world) if p != k})
    torch.cuda.synchronize()

    def body(k, comm):
        for ci in range(len(combos)):
            src, gathered, xs, xr = bufs[ci, k]
            comm.all_gather(gathered.view, src.view)
            comm.exchange({p: g.view for p, g in xs.items()}, {p: g.view for p, g in xr.items()})

    _comm_threads(torch, world, body)
    for ci, (n, so, do) in enumerate(combos):
        want = torch.cat([_payload(torch, n, 10 * ci + p) for p in range(world)])
        for k in range(world):
            src, gathered, xs, xr = bufs[ci, k]
            what = f"{n} bytes, offsets {so} -> {do}, rank {k}"
            gathered.check(want, "all_gather of " + what)
            src.check(_payload(torch, n, 10 * ci + k), "the source of " + what)
            for p, g in xr.items():
                g.check(_payload(torch, n, 1000 + 100 * ci + 10 * p + k), f"exchange of {what} from rank {p}")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n,off", [(4096 * 256 * 16 + 16, 0), (4096 * 256 + 1, 1)], ids=["vector", "bytes"])
def test_comm_grid_stride(n, off):
    """One work item more than 4096 blocks of 256 lanes hold, on the 16-byte path and on the byte path: the copy
    kernel's grid-stride loop takes a second trip."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    src = [_Guarded(torch, n, off) for _ in range(2)]
    dst = [_Guarded(torch, n, off) for _ in range(2)]
    for k in range(2):
        src[k].view.copy_(_payload(torch, n, k))
        assert (src[k].view.data_ptr() % 16 == 0) == (off == 0)
    torch.cuda.synchronize()
    _comm_threads(torch, 2, lambda k, comm: comm.exchange({1 - k: src[k].view}, {1 - k: dst[k].view}))
    for k in range(2):
        dst[k].check(_payload(torch, n, 1 - k), f"rank {k}")


@pytest.mark.timeout(120)
def test_comm_all_gather_beyond_sixteen_segments():
    """An all-gather reads every rank's block, its own included: at 17 ranks the segment list exceeds kMaxCopySegs = 16
    and LocalComm::copy_all issues a second launch for the seventeenth (an exchange reaches 17 only at 18 ranks).
    Five bytes per rank at offset 1."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    world, n = 17, 5
    src = [_Guarded(torch, n, 1) for _ in range(world)]
    dst = [_Guarded(torch, world * n, 1) for _ in range(world)]
    for k in range(world):
        src[k].view.copy_(_payload(torch, n, k))
    torch.cuda.synchronize()
    _comm_threads(torch, world, lambda k, comm: comm.all_gather(dst[k].view, src[k].view))
    want = torch.cat([_payload(torch, n, k) for k in range(world)])
    for k in range(world):
        dst[k].check(want, f"rank {k}")


@pytest.mark.timeout(120)
def test_comm_zero_byte_send_beside_others():
    """Rank 0 sends nothing to rank 1 and 33 bytes to rank 2 in one exchange (a rank without rows sends no AO band);
    ranks 1 and 2 send 7 and 16 bytes to rank 0.  Every non-empty transfer arrives, nothing else is written."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sizes = {(0, 1): 0, (0, 2): 33, (1, 0): 7, (2, 0): 16, (1, 2): 0, (2, 1): 1}
    src = {e: _Guarded(torch, n, 1) for e, n in sizes.items()}
    dst = {e: _Guarded(torch, n, 1) for e, n in sizes.items()}
    for i, (e, n) in enumerate(sizes.items()):
        src[e].view.copy_(_payload(torch, n, i))
    torch.cuda.synchronize()

    def body(k, comm):
        comm.exchange({q: src[(p, q)].view for (p, q) in sizes if p == k},
                      {p: dst[(p, q)].view for (p, q) in sizes if q == k})

    _comm_threads(torch, 3, body)
    for i, (e, n) in enumerate(sizes.items()):
        dst[e].check(_payload(torch, n, i), f"rank {e[0]} -> rank {e[1]}")
