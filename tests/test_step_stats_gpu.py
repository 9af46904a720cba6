"""GPU: ops.step_stats (ws_step_stats, csrc/stats.hip) -- the record of a training step's log line.

`correct` is an integer and is compared for equality with torch's own `(argmax(logits, 1) == target).sum()` on the same
device (KPFCNN.accuracy's numerator, models/architectures.py:386-399); the three floats are bit copies and are compared as
int32 words.  No tolerance anywhere.

Shapes: N in {0, 1, 255, 256, 257} around the workgroup's 256 rows and N = WS_STEP_STATS_BLOCKS * 256 + 1, the first size at
which the grid-stride loop makes a second trip; C in {1, 9, WS_STEP_STATS_MAX_C}; row pitch C and C + 3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _abi():
    from weasal_amd import _lib
    return _lib.ABI.constants["WS_STEP_STATS_BLOCKS"], _lib.ABI.constants["WS_STEP_STATS_MAX_C"]


def _cases():
    blocks, max_c = 256, 64               # asserted against the header in test_constants_are_the_headers
    return [(n, c, pad) for n in (0, 1, 255, 256, 257, blocks * 256 + 1) for c in (1, 9, max_c) for pad in (0, 3)]


def test_constants_are_the_headers():
    assert _abi() == (256, 64)


def _logits(n, c, pad, seed, dev):
    """[n, c] view of a [n, c + pad] buffer.  From 255 rows on, the first rows hold: exact ties at the maximum in the first,
    middle and last positions, a row of equal values, +inf / -inf entries, a row of -inf, and rows with one and two NaN"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn((n, c + pad), generator=g, dtype=torch.float32)
    if pad:
        buf[:, c:] = 1e30                 # the padding would win every row if it were read
    x = buf[:, :c]
    inf, nan = float("inf"), float("nan")
    if n >= 255:
        m, last = c // 2, c - 1
        x[0, [0, min(1, last)]] = 7.0                       # tie at the first position
        x[1, [m, last]] = 7.0                               # tie middle / last
        x[2, [max(last - 1, 0), last]] = 7.0                # tie at the last position
        x[3, :] = 0.25                                      # all equal
        x[4, m] = inf
        x[5, :] = -inf
        x[5, last] = -3.0
        x[6, :] = -inf                                      # all -inf: the first
        x[7, [0, last]] = inf                               # two +inf
        x[8, m] = nan                                       # NaN beats the larger entries around it
        x[8, last] = 9.0
        x[9, [m, last]] = nan                               # two NaN: the first
        x[9, 0] = inf
        x[10, last] = nan
    return buf.to(dev)[:, :c]


def _labels(pred, n_values, seed, null_lut):
    """about half the rows carry the value that maps to torch's prediction, the rest random values; then ignored, negative
    and out-of-table values are strewn in"""
    n = pred.shape[0]
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, n_values, (n,), generator=g, dtype=torch.int64)
    hit = torch.rand(n, generator=g) < 0.5
    lab = torch.where(hit, pred.cpu(), lab)
    odd = torch.randint(0, 12, (n,), generator=g)
    lab = torch.where(odd == 0, torch.full_like(lab, -1), lab)
    lab = torch.where(odd == 1, torch.full_like(lab, n_values + 5), lab)
    lab = torch.where(odd == 2, torch.full_like(lab, 1 << 40), lab)
    lab = torch.where(odd == 3, torch.full_like(lab, -(1 << 40)), lab)
    return lab


def _record(ring, row):
    return ring[row].cpu().numpy().copy()


@pytest.mark.parametrize("n, c, pad", _cases())
def test_correct_equals_torch(gpu, n, c, pad):
    from weasal_amd import ops
    x = _logits(n, c, pad, 100 + c + pad, gpu)
    assert x.stride(0) == c + pad
    pred = torch.argmax(x, dim=1) if n else torch.zeros(0, dtype=torch.int64, device=gpu)
    ring = torch.full((3, 4), -7, dtype=torch.int32, device=gpu)
    # ---- the NULL-table form: labels are positions, < 0 and >= C never count
    lab = _labels(pred, c, 5, True).to(gpu)
    target = torch.where((lab >= 0) & (lab < c), lab, torch.full_like(lab, -1))
    want = int((pred == target).sum())
    ops.step_stats(ring, 1, x, lab)
    got = _record(ring, 1)
    print("n=%d c=%d pitch=%d positions: correct %d of %d" % (n, c, c + pad, got[3], n))
    assert got[3] == want and (got[:3] == 0).all()
    assert (ring[[0, 2]].cpu().numpy() == -7).all()
    # ---- through a table: value v -> position perm[v], two values ignored, anything outside the table ignored
    values = c + 2
    perm = torch.randperm(values, generator=torch.Generator().manual_seed(9))
    table = torch.where(perm < c, perm, torch.full_like(perm, -1))
    lut = torch.cat([table, torch.tensor([-1])]).to(torch.int64).to(gpu)
    inverse = torch.zeros(c, dtype=torch.int64)
    inverse[table[table >= 0]] = torch.nonzero(table >= 0).reshape(-1)
    lab = _labels(inverse.to(gpu)[pred].cpu() if n else pred.cpu(), values, 6, False).to(gpu)
    inside = (lab >= 0) & (lab < values)
    target = torch.where(inside, lut[torch.where(inside, lab, torch.zeros_like(lab))], torch.full_like(lab, -1))
    want = int((pred == target).sum())
    ops.step_stats(ring, 2, x, lab, lut)
    got2 = _record(ring, 2)
    print("n=%d c=%d pitch=%d table:     correct %d of %d" % (n, c, c + pad, got2[3], n))
    assert got2[3] == want
    if n >= 255:
        assert 0 < want < n
    assert (_record(ring, 1) == got).all() and (_record(ring, 0) == -7).all()


def test_special_rows_one_by_one(gpu):
    """the tie / inf / NaN rows of _logits, each as a batch of its own with the label torch predicts: every one counts"""
    from weasal_amd import ops
    for c in (9, 64):
        x = _logits(255, c, 0, 3, gpu)[:11]
        pred = torch.argmax(x, dim=1)
        m, last = c // 2, c - 1
        assert pred.cpu().tolist() == [0, m, last - 1, 0, m, last, 0, 0, m, m, last]
        ring = torch.zeros((11, 4), dtype=torch.int32, device=gpu)
        for r in range(11):
            ops.step_stats(ring, r, x[r:r + 1], pred[r:r + 1])
        assert ring[:, 3].cpu().tolist() == [1] * 11
        for r in range(11):
            ops.step_stats(ring, r, x[r:r + 1], (pred[r:r + 1] + 1) % c)
        assert ring[:, 3].cpu().tolist() == [0] * 11


def test_floats_are_bit_copies_and_rows_stay(gpu):
    from weasal_amd import ops
    words = np.array([0x80000000, 0x7fc01234, 0x00000001, 0x3f800001, 0xff800000], dtype=np.uint32).view(np.int32)
    dev = torch.from_numpy(words.copy()).to(gpu).view(torch.float32)
    x = _logits(257, 9, 3, 1, gpu)
    lab = torch.argmax(x, dim=1)
    ring = torch.full((4, 4), 0x5a5a5a5a, dtype=torch.int32, device=gpu)
    ops.step_stats(ring, 2, x, lab, None, dev[0:1], dev[1:2], dev[2:3])
    got = ring.cpu().numpy()
    assert got[2].tolist() == [words[0], words[1], words[2], 257]
    assert (got[[0, 1, 3]] == 0x5a5a5a5a).all()
    ops.step_stats(ring, 0, x, lab, None, None, dev[3], None)              # a 0-dim scalar; NULL logs +0.0
    ops.step_stats(ring, 3, x, lab, None, dev[4:5], None, dev[0:1])
    got = ring.cpu().numpy()
    assert got[0].tolist() == [0, words[3], 0, 257] and got[3].tolist() == [words[4], 0, words[0], 257]
    assert got[2].tolist() == [words[0], words[1], words[2], 257] and (got[1] == 0x5a5a5a5a).all()


def test_two_runs_give_equal_bytes(gpu):
    from weasal_amd import ops
    blocks, _ = _abi()
    n = blocks * 256 * 2 + 77                                                   # three trips for some workgroups
    x = _logits(n, 9, 0, 2, gpu)
    lab = _labels(torch.argmax(x, dim=1), 9, 4, True).to(gpu)
    loss = torch.tensor([1.25], device=gpu)
    rings = []
    for _ in range(2):
        ring = torch.zeros((2, 4), dtype=torch.int32, device=gpu)
        for row in (0, 1, 0):                                                   # row 0 written twice: zeroed by the call
            ops.step_stats(ring, row, x, lab, None, loss, None, None)
        rings.append(ring.cpu().numpy().tobytes())
    assert rings[0] == rings[1]
    rec = np.frombuffer(rings[0], np.int32).reshape(2, 4)
    target = torch.where((lab >= 0) & (lab < 9), lab, torch.full_like(lab, -1))
    assert rec[0, 3] == rec[1, 3] == int((torch.argmax(x, dim=1) == target).sum())


def test_refusals(gpu):
    from weasal_amd import _lib, ops
    ring = torch.zeros((2, 4), dtype=torch.int32, device=gpu)
    lab = torch.zeros(4, dtype=torch.int64, device=gpu)
    with pytest.raises(_lib.WeasalHipError, match="c <= 64"):
        ops.step_stats(ring, 0, torch.zeros((4, 65), device=gpu), lab)
    for row in (-1, 2):
        with pytest.raises(_lib.WeasalHipError, match="outside the ring"):
            ops.step_stats(ring, row, torch.zeros((4, 9), device=gpu), lab)
    with pytest.raises(_lib.WeasalHipError):
        ops.step_stats(ring, 0, torch.zeros((4, 9)), lab.cpu())
    with pytest.raises(_lib.WeasalHipError, match="float32 scalar"):
        ops.step_stats(ring, 0, torch.zeros((4, 9), device=gpu), lab, None, torch.zeros(2, device=gpu))
    assert int(ring.abs().sum()) == 0
