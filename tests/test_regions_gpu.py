"""GPU: the per-sphere regions of the weak-label sampler (weasal_amd.regions, csrc/regions.hip) against the CPU restatement
tests/regions_ref.py and golden g17_regions.npz, the region means against float64 with per-element rounding bounds, and the
device path of KPFCNN_mprm.region_mprm_loss / trainer.train_step_weak against the list path.

The cut is integers and 0/1 rows (and one correctly rounded 1 / n): it is compared for equality.  The means are float32 sums:
  forward   |err| <= (n + 2) * 2^-24 * (sum |x_i| / n)          n - 1 additions in any order, one rounding of 1 / n, one product
  backward  |err| <= (m + 2) * 2^-24 * sum_r |g_r| * inv_len_r  m products, m - 1 additions, the rounding of inv_len
Loss and step: 1e-4 relative, the bar the README states for fp32 activations and gradients."""
import copy

import numpy as np
import pytest
import torch

import anchors_ref
import regions_ref
from conftest import golden
from test_regions_cpu import golden_anchor_set, golden_record

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def device_set(aset, dev):
    """(lists, lb, centres) -> weasal_amd.anchors.AnchorSet made directly from the arrays"""
    from weasal_amd.anchors import AnchorSet
    lists, lb, centres = aset
    ptr, idx = regions_ref.csr(lists)
    lb = np.asarray(lb, np.int64)
    assert lb.ndim == 2 and lb.shape[0] == len(lists)
    bits = regions_ref.pack_bits(lb) if len(lists) else np.zeros(0, np.uint32)
    return AnchorSet(np.asarray(centres, np.float64).reshape(-1, 3), torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev),
                     torch.from_numpy(bits).to(dev), lb, np.arange(len(lists), dtype=np.int64), len(lists))


def device_cut(b, dev, labels=None):
    from weasal_amd import regions
    sets = [device_set(a, dev) for a in b["anchor_sets"]]
    lab = b["labels"] if labels is None else labels
    return regions.cut_regions(sets, b["cloud_inds"], b["centres"], torch.from_numpy(b["input_inds"]).to(dev), b["lengths"],
                               torch.from_numpy(np.asarray(lab, np.int64)).to(dev), b["in_radius"], b["sub_radius"], b["n_class"])


def ref_cut(b):
    return regions_ref.cut(b["anchor_sets"], b["cloud_inds"], b["centres"], b["input_inds"], b["lengths"], b["labels"], b["in_radius"],
                           b["sub_radius"], b["n_class"])


def assert_cut_equal(sr, want, n):
    assert len(sr) == len(want["ptr"]) - 1 and sr.nnz == len(want["idx"])
    for name in ("ptr", "idx", "sphere", "anchor", "lb", "inv_len", "cloud_lb"):
        got = getattr(sr, name).cpu().numpy()
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
    t_ptr, t_reg = regions_ref.transpose(want["ptr"], want["idx"], n)
    assert np.array_equal(sr.t_ptr.cpu().numpy(), t_ptr) and sr.t_ptr.dtype == torch.int64
    assert np.array_equal(sr.t_reg.cpu().numpy(), t_reg) and sr.t_reg.dtype == torch.int32
    assert np.array_equal(sr.reg.cpu().numpy(), np.repeat(np.arange(len(sr), dtype=np.int32), np.diff(want["ptr"])))


@pytest.fixture(scope="module")
def edge(gpu):
    b = regions_ref.edge_batch()
    return b, ref_cut(b), device_cut(b, gpu)


def test_fixture_holds_every_case():
    b = regions_ref.edge_batch()
    want = ref_cut(b)
    cases, lens = b["cases"], np.diff(want["ptr"])
    row_off = np.concatenate([[0], np.cumsum(b["lengths"])])
    kept = {(int(s), int(a)): int(n) for s, a, n in zip(want["sphere"], want["anchor"], lens)}
    tile0 = b["anchor_sets"][0]
    cand0 = set(regions_ref.candidates(tile0[2], b["centres"][0], regions_ref.search_radius(b["in_radius"], b["sub_radius"])).tolist())
    assert b["tiles"][0][0].shape[0] > 1400 and b["tiles"][1][0].shape[0] < 100
    assert int(b["lengths"].sum()) % 64 != 0
    assert not any(s == 2 for s, _ in kept) and len(regions_ref.candidates(tile0[2], b["centres"][2], 5.99)) == 0      # no candidate
    assert cases["outside"] in cand0 and (0, cases["outside"]) not in kept                     # members all outside the sphere
    assert cases["row0_only"] in cand0 and (0, cases["row0_only"]) not in kept                 # only row 0
    r = [i for i in range(len(lens)) if want["sphere"][i] == 0 and want["anchor"][i] == cases["row0_more"]][0]
    assert want["idx"][want["ptr"][r]] == row_off[0] and lens[r] == 6                          # row 0 and others
    assert kept[(0, cases["single"])] == 1                                                     # one member, not row 0
    assert [kept[(0, cases[k])] for k in ("n64", "n65", "n257", "n1100")] == [64, 65, 257, 1100]
    assert kept[(0, cases["partly"])] == 20 < len(tile0[0][cases["partly"]])                   # partly outside
    assert 0 < kept[(4, cases["n1100"])] < 1100                                                # (and so for the shifted sphere)
    assert (0, cases["on_radius"]) in kept and cases["ulp_out"] not in cand0                   # on the radius / an ulp outside
    assert (4, cases["ulp_out"]) in kept
    assert list(b["cloud_inds"]).count(0) == 3 and len(set(b["cloud_inds"].tolist())) == 3     # a tile twice; several tiles
    assert len(b["anchor_sets"][2][0]) == 0 and b["cloud_inds"][3] == 2                        # an empty AnchorSet
    assert kept[(0, cases["repeat"])] == kept[(0, cases["n64"])] == 64                         # an anchor repeated in its set
    assert np.array_equal(tile0[0][cases["repeat"]], tile0[0][cases["n64"]])
    assert (1, 0) in kept and (1, 1) not in kept                                               # the small tile: {row 0} again
    assert cases["far"] not in {a for _, a in kept}


def test_cut_equals_the_restatement(edge):
    b, want, sr = edge
    assert_cut_equal(sr, want, int(b["lengths"].sum()))
    region, region_lb = sr.to_lists()
    for s in range(len(b["lengths"])):
        assert len(region[s]) == len(want["region"][s])
        for a, w, la, lw in zip(region[s], want["region"][s], region_lb[s], want["region_lb"][s]):
            assert np.array_equal(a, w) and np.array_equal(la, lw)


def test_cut_is_deterministic(edge, gpu):
    b, _, sr = edge
    again = device_cut(b, gpu)
    for name in ("ptr", "idx", "reg", "sphere", "anchor", "lb", "inv_len", "t_ptr", "t_reg", "cloud_lb"):
        assert getattr(sr, name).cpu().numpy().tobytes() == getattr(again, name).cpu().numpy().tobytes(), name


def test_golden_spheres_as_sets(gpu):
    from weasal_amd import regions
    g = golden("g17_regions.npz")
    points, labels = anchors_ref.golden_cloud()
    aset = device_set(golden_anchor_set(g), gpu)
    in_radius, sub_radius, nc = float(g["in_radius"]), float(g["sub_radius"]), int(g["n_class"])
    inds = [regions_ref.sphere_inds(points, c, in_radius) for c in g["centres"]]
    lengths = [len(i) for i in inds]
    assert lengths[-1] == 0                                                                    # the sphere far outside the cloud
    stacked = np.concatenate(inds)
    sr = regions.cut_regions([aset], np.zeros(len(inds), np.int64), g["centres"], torch.from_numpy(stacked).to(gpu), lengths,
                             torch.from_numpy(labels[stacked].astype(np.int64)).to(gpu), in_radius, sub_radius, nc)
    ptr, idx, sph, lb = (t.cpu().numpy() for t in (sr.ptr, sr.idx, sr.sphere, sr.lb))
    for k in range(len(inds)):
        mine = sorted((tuple(stacked[idx[ptr[r]:ptr[r + 1]]]), tuple(int(v) for v in lb[r])) for r in range(len(sr)) if sph[r] == k)
        assert mine == golden_record(g, k), k
    assert len(sr) == 17 + 16 + 12


def test_bad_label_raises(edge, gpu):
    b = edge[0]
    for bad in (-1, b["n_class"]):
        lab = b["labels"].copy()
        lab[len(lab) // 2] = bad
        with pytest.raises(ValueError, match="outside"):
            device_cut(b, gpu, labels=lab)


@pytest.fixture(scope="module")
def maps(edge, gpu):
    b = edge[0]
    n = int(b["lengths"].sum())
    rng = np.random.RandomState(5)
    x = (rng.standard_normal((n, 36)) * rng.choice([1e-2, 1.0, 30.0], size=(n, 1))).astype(np.float32)
    return x, torch.from_numpy(x).to(gpu)


def test_region_mean_forward_bound(edge, maps, gpu):
    from weasal_amd import ops
    _, want, sr = edge
    x, dx = maps
    out = torch.full((len(sr), 36), float("nan"), dtype=torch.float32, device=gpu)
    ops.region_mean_fwd(dx, sr, out=out)
    ref, mag = regions_ref.region_mean64(x, want["ptr"], want["idx"])
    n = np.diff(want["ptr"]).astype(np.float64)[:, None]
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    print("forward W=36: worst err / bound = %.3f" % float((err / ((n + 2) * U * mag)).max()))
    assert (err <= (n + 2) * U * mag).all()
    assert ops.region_mean_fwd(dx, sr).cpu().numpy().tobytes() == got.tobytes()                # the same bytes again


def test_region_mean_width_256_and_257(gpu):
    """a small case at the widest supported shape (one row of the block per pass), and one column more"""
    from weasal_amd import ops, regions
    lists = [np.array([0, 3, 4], np.int64), np.arange(1, 70, dtype=np.int64), np.array([68], np.int64)]
    aset = (lists, np.eye(3, 9, dtype=np.int64), np.zeros((3, 3)))
    inds = np.arange(0, 69, dtype=np.int64)
    sr = regions.cut_regions([device_set(aset, gpu)], [0], np.zeros((1, 3)), torch.from_numpy(inds).to(gpu), [69],
                             torch.zeros(69, dtype=torch.int64, device=gpu), 10.0, 4.0, 9)
    want = regions_ref.cut([aset], [0], np.zeros((1, 3)), inds, [69], np.zeros(69, np.int64), 10.0, 4.0, 9)
    assert_cut_equal(sr, want, 69)
    assert np.diff(want["ptr"]).tolist() == [3, 68, 1]
    x = np.random.RandomState(8).standard_normal((69, 256)).astype(np.float32)
    out = torch.full((3, 256), float("nan"), dtype=torch.float32, device=gpu)
    ops.region_mean_fwd(torch.from_numpy(x).to(gpu), sr, out=out)
    ref, mag = regions_ref.region_mean64(x, want["ptr"], want["idx"])
    n = np.diff(want["ptr"]).astype(np.float64)[:, None]
    assert (np.abs(out.cpu().numpy().astype(np.float64) - ref) <= (n + 2) * U * mag).all()
    g = np.random.RandomState(9).standard_normal((3, 256)).astype(np.float32)
    dx = torch.full((69, 256), float("nan"), dtype=torch.float32, device=gpu)
    ops.region_mean_bwd(torch.from_numpy(g).to(gpu), sr, out=dx)
    dref, dmag, m = regions_ref.region_mean_grad64(g, want["ptr"], want["idx"], 1.0 / np.diff(want["ptr"]), 69)
    assert (np.abs(dx.cpu().numpy().astype(np.float64) - dref) <= (m[:, None] + 2) * U * dmag).all()
    wide = torch.zeros((69, 257), dtype=torch.float32, device=gpu)
    with pytest.raises(ValueError, match="256"):
        ops.region_mean(wide, sr)
    with pytest.raises(ValueError, match="256"):
        ops.region_mean_fwd(wide, sr)


def test_region_mean_backward_bound(edge, maps, gpu):
    from weasal_amd import ops
    b, want, sr = edge
    n = int(b["lengths"].sum())
    g = np.random.RandomState(6).standard_normal((len(sr), 36)).astype(np.float32)
    dg = torch.from_numpy(g).to(gpu)
    out = torch.full((n, 36), float("nan"), dtype=torch.float32, device=gpu)
    ops.region_mean_bwd(dg, sr, out=out)
    got = out.cpu().numpy()
    ref, mag, m = regions_ref.region_mean_grad64(g, want["ptr"], want["idx"], 1.0 / np.diff(want["ptr"]), n)
    assert (m == 0).any() and m.max() >= 3
    assert (got[m == 0] == 0).all() and not np.signbit(got[m == 0]).any()                      # rows in no region: exact zeros
    err = np.abs(got.astype(np.float64) - ref)
    bound = (m[:, None] + 2) * U * mag
    print("backward W=36: worst err / bound = %.3f" % float((err[m > 0] / bound[m > 0]).max()))
    assert (err <= bound).all()
    # through autograd, twice: the same bytes
    grads = []
    for _ in range(2):
        x = maps[1].clone().requires_grad_(True)
        ops.region_mean(x, sr).backward(dg)
        grads.append(x.grad.cpu().numpy())
    assert grads[0].tobytes() == grads[1].tobytes() == got.tobytes()


class _Loss:
    """what region_mprm_loss uses of the network: the criterion"""
    criterion_multi = torch.nn.BCEWithLogitsLoss()


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_region_loss_device_path_list_path_and_float64(edge, gpu):
    from weasal_amd.architectures import KPFCNN_mprm
    b, want, sr = edge
    n, c, k = int(b["lengths"].sum()), b["n_class"], 4
    rng = np.random.RandomState(12)
    cams = [rng.standard_normal((n, c)).astype(np.float32) * 3 for _ in range(k)]
    # float64 on the CPU
    c64 = [torch.from_numpy(m).double().requires_grad_(True) for m in cams]
    x64 = torch.cat(c64, dim=1)
    idx, ptr = torch.from_numpy(want["idx"]), want["ptr"]
    avg = torch.stack([x64[idx[ptr[r]:ptr[r + 1]]].mean(dim=0) for r in range(len(ptr) - 1)])
    lb64 = torch.from_numpy(want["lb"]).double()
    loss64 = sum(torch.nn.functional.binary_cross_entropy_with_logits(avg[:, i * c:(i + 1) * c], lb64) for i in range(k))
    loss64.backward()
    region, region_lb = sr.to_lists()
    for tag, args in (("device", (sr, None, None)), ("lists", (region, region_lb, b["lengths"]))):
        dc = [torch.from_numpy(m).to(gpu).requires_grad_(True) for m in cams]
        loss = KPFCNN_mprm.region_mprm_loss(_Loss(), dc, *args)
        loss.backward()
        worst = max(_rel(a.grad, w.grad) for a, w in zip(dc, c64))
        got, ref = float(loss.detach()), float(loss64.detach())
        print("%s path: loss rel %.2e, worst gradient rel %.2e" % (tag, abs(got - ref) / ref, worst))
        assert abs(got - ref) <= 1e-4 * ref, tag
        assert worst < 1e-4, tag


def test_weak_label_step_with_device_regions(gpu):
    """the small shapes of test_weak_label_gpu.test_weak_label_step_vs_golden: the g10 batch, every sphere its own tile, anchors
    built on its points by weasal_amd.anchors; one net steps on the SphereRegions, a deep copy on its to_lists()"""
    from weasal_amd import anchors, config as wcfg, regions
    from weasal_amd.architectures import KPFCNN_mprm
    from weasal_amd.pyramid import PyramidBatch
    from weasal_amd.trainer import make_optimizer, train_step_weak
    g = golden("g10_mprm.npz")

    class Cfg(wcfg.Vaihingen3DWLConfig):
        dataset = "GoldenWL"
        num_classes = 6
        first_subsampling_dl = 0.3
        first_features_dim = 16
        class_w = []
        weight_decay = 1e-3
    cfg = Cfg()
    L, in_radius, sub_radius = 3, 3.0, 1.0

    def make_batch():
        li = [torch.from_numpy(g["points_%d" % l]).to(gpu) for l in range(L)]
        li += [torch.from_numpy(g["neighbors_%d" % l].astype(np.int64)).to(gpu) for l in range(L)]
        li += [torch.from_numpy(g["pools_%d" % l].astype(np.int64)).to(gpu) for l in range(L)]
        li += [torch.from_numpy(g["upsamples_%d" % l].astype(np.int64)).to(gpu) for l in range(L)]
        li += [torch.from_numpy(g["lengths_%d" % l].astype(np.int32)).to(gpu) for l in range(L)]
        li += [torch.from_numpy(g["features"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu)]
        batch = PyramidBatch(li)
        batch.center_pts = torch.from_numpy(g["center_pts"]).to(gpu)
        return batch
    lengths = g["lengths_0"].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    labels = torch.from_numpy(g["labels"].astype(np.int64)).to(gpu)
    pts = torch.from_numpy(g["points_0"]).to(gpu)
    sets = []
    for s in range(len(lengths)):
        p, l = pts[offs[s]:offs[s + 1]].contiguous(), labels[offs[s]:offs[s + 1]]
        a = anchors.anchors_with_points(p, l, anchors.get_anchors(p, sub_radius, 'reduced'), sub_radius, cfg.num_classes)
        sets.append(anchors.update_anchors(a, p, sub_radius))
    inds = torch.cat([torch.arange(int(n), device=gpu) for n in lengths])
    sr = regions.cut_regions(sets, np.arange(len(lengths)), np.zeros((len(lengths), 3)), inds, lengths, labels, in_radius, sub_radius,
                             cfg.num_classes)
    assert len(sr) >= 4 and set(sr.sphere.cpu().tolist()) == {0, 1}
    np.random.seed(0)
    torch.manual_seed(0)
    net = KPFCNN_mprm(cfg, np.arange(6), []).to(gpu).train()
    net.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd0/")}, strict=False)
    twin = copy.deepcopy(net)
    losses = []
    for model, region in ((net, sr), (twin, None)):
        batch = make_batch()
        if region is None:
            batch.region, batch.region_lb = sr.to_lists()
        else:
            batch.region, batch.region_lb = region, None
        loss, _ = train_step_weak(model, make_optimizer(model, cfg), batch, cfg)
        losses.append(float(loss.detach()))
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1])
    moved = 0
    for (name, a), (_, w) in zip(net.named_parameters(), twin.named_parameters()):
        assert _rel(a, w) < 1e-4, name
        moved += int(not torch.equal(w.detach().cpu(), torch.from_numpy(g["sd0/" + name]))) if "sd0/" + name in g.files else 0
    assert moved > 10                                                                           # (the step did move the twin)
    # a batch whose cut is empty is the skipped batch
    far = regions.cut_regions(sets, np.arange(len(lengths)), np.full((len(lengths), 3), 500.0), inds, lengths, labels, in_radius,
                              sub_radius, cfg.num_classes)
    assert len(far) == 0 and far.ptr.cpu().tolist() == [0] and int(far.t_ptr.max()) == 0
    batch = make_batch()
    batch.region, batch.region_lb = far, None
    assert train_step_weak(net, make_optimizer(net, cfg), batch, cfg) == (None, None)


def test_sampler_cuts_the_regions_of_its_last_batch(gpu):
    import sampler_ref
    from weasal_amd import anchors
    from weasal_amd.sampler import SphereSampler

    class Cfg:
        in_features_dim = 3
        augment_rotation = 'vertical'
        augment_scale_anisotropic = True
        augment_scale_min = 0.9
        augment_scale_max = 1.1
        augment_symmetries = [True, False, False]
        augment_noise = 0.0
        batch_num = 4
        in_radius = 3.0
        sub_radius = 1.0
        num_classes = 9
    cfg = Cfg()
    clouds, sets, host_sets = [], [], []
    for seed, n in ((31, 20000), (32, 9000)):
        p, l = sampler_ref.slab_cloud(seed, n, 9.0, 1.0, 0.4)
        p, l = torch.from_numpy(p).to(gpu), torch.from_numpy(l).to(gpu)
        a = anchors.anchors_with_points(p, l, anchors.get_anchors(p, cfg.sub_radius, 'reduced'), cfg.sub_radius, cfg.num_classes)
        a = anchors.update_anchors(a, p, cfg.sub_radius)
        clouds.append((p, l))
        sets.append(a)
        ptr, idx = a.ptr.cpu().numpy(), a.idx.cpu().numpy()
        host_sets.append(([idx[ptr[k]:ptr[k + 1]] for k in range(len(a))], a.lb, a.centres))
    s = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=5, max_spheres=8, batch_limit=3000)
    with pytest.raises(ValueError, match="set_anchors"):
        s.cut_regions()
    s.set_anchors(sets)
    with pytest.raises(ValueError, match="sample"):
        s.cut_regions()
    for _ in range(2):
        syncs, cuts = s._sync_count, s._region_sync_count
        out = s.sample(capacity_rows=100000)
        assert s._sync_count - syncs == 1 and s._region_sync_count == cuts                     # sample(): its single read
        sr = s.cut_regions()
        assert s._sync_count - syncs == 1 and s._region_sync_count - cuts == 1                 # the cut: one read of its own
        labels, lengths, cloud_inds, input_inds = out[2].cpu().numpy(), out[3], out[6].cpu().numpy(), out[8].cpu().numpy()
        want = regions_ref.cut(host_sets, cloud_inds, s.last_centres, input_inds, lengths, labels, cfg.in_radius, cfg.sub_radius,
                               cfg.num_classes)
        assert len(sr) > 0 and len(lengths) >= 2
        assert_cut_equal(sr, want, int(np.sum(lengths)))
