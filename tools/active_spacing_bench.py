"""active.select_points with and without a minimum spacing (`al_min_spacing`), the sibling of tools/active_bench.py: one
tile-sized cloud (300 000 points, votes from tests/active_ref.synthetic_votes like there), k = 5000 (the Vaihingen
pseudo-label configuration's added_labels_per_epoch), with no used ids and with the 5000 of one earlier iteration.

The coordinates are a 0.24 m grid with jitter (a sub-cloud's spacing); the spacing is 0.5 m, two grid pitches.  Both arms
run on the same votes, alternating, five times each after a warm-up; a time is the wall time of the call plus the host read
of the k ids.  The spaced arm also reports its runs (`passes`), the candidates handed to the walk (`consumed`) and the
stream time of the two spaced launches alone (HIP events around ws_al_spaced_select on the candidates of that run)."""
import ctypes as C, json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import active_ref
from weasal_amd import _lib, active

N, K, SPACING, REPS = 300_000, 5000, 0.5, 5
dev = torch.device("cuda:0")
class_w = np.ones(9)
lib = _lib.lib()


class Votes:
    def __init__(self, probs):
        self.probs = [probs]


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


rng = np.random.default_rng(7)
side = int(np.ceil(np.sqrt(N)))
gx, gy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
xyz = np.stack([gx.reshape(-1)[:N] * 0.24, gy.reshape(-1)[:N] * 0.24, np.zeros(N)], 1) + rng.uniform(-0.1, 0.1, size=(N, 3))
points = torch.from_numpy(xyz.astype(np.float32)).to(dev)
votes = Votes(torch.from_numpy(active_ref.synthetic_votes(1, N, 9)).to(dev))
rows = []
for n_used in (0, K):
    used = rng.choice(N, size=n_used, replace=False).astype(np.int64)
    plain = lambda: active.select_points(votes, 0, class_w, used, K).cpu()
    spaced = lambda: active.select_points(votes, 0, class_w, used, K, points=points, min_spacing=SPACING).cpu()
    for _ in range(3):
        plain(); spaced()
    t_plain, t_spaced = [], []
    for _ in range(REPS):                                          # alternating
        t_plain.append(wall(plain)); t_spaced.append(wall(spaced))
    before = lib.ws_launch_count(); plain(); l_plain = lib.ws_launch_count() - before
    before = lib.ws_launch_count(); ids = spaced(); l_spaced = lib.ws_launch_count() - before
    passes, consumed = active.last_spaced["passes"], active.last_spaced["consumed"]
    # the two spaced launches alone, on the first run's candidates
    score = active.point_scores(votes.probs[0], class_w)[2]
    m = min(N - n_used, max(active.SPACED_PREFIX_FACTOR * K, active.SPACED_PREFIX_MIN))
    cand = active.top_k(score, m, used)
    out, state = torch.empty(K, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.ws_al_spaced_scratch_bytes(m, n_used, K), dtype=torch.uint8, device=dev)
    alone = []
    for _ in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        _lib.check(lib.ws_al_spaced_select(_lib.ptr(points), 0, N, _lib.ptr(cand), m, C.c_void_p(used.ctypes.data), n_used, SPACING, K,
                                           _lib.ptr(out), _lib.ptr(state), 0, _lib.ptr(scratch), _lib.current_stream()))
        e1.record(); torch.cuda.synchronize()
        alone.append(e0.elapsed_time(e1))
    accepted, walked = state.cpu().tolist()
    rows.append(dict(n=N, k=K, used=n_used, spacing=SPACING, plain_ms=spread(t_plain), spaced_ms=spread(t_spaced),
                     plain_ms_all=t_plain, spaced_ms_all=t_spaced, launches_plain=int(l_plain), launches_spaced=int(l_spaced),
                     passes=passes, candidates_handed_over=consumed, candidates_walked=walked, accepted=accepted,
                     spaced_launches_stream_ms=spread(alone[1:]), ids_equal_direct=bool(torch.equal(out.cpu(), ids))))
    print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(dict(rows=rows), open(os.path.join(REPO, "bench_outputs", "active_spacing_bench.json"), "w"))
