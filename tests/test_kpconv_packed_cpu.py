"""The scope of the packed table walk of K4, asked of its reporter without a device: ws_kpconv_gather_bwd_x_packed_variant
formats the plan the launcher of ws_kpconv_gather_bwd_x_packed follows (kpconv.hip: bwd_x_packed_plan).  It names
kpconv_gather_bwd_x_packed_kernel only for f32 rows in float4 pieces (ci % 4 == 0, dwf and dx 16-byte aligned), a rigid
kernel with linear influence and sum aggregation, fewer queries than supports and a mean in-degree nq * h / ns of at most
PACK_MEAN_MAX (read from the source), with G from the row width as in K4; everywhere else it answers "none"."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(REPO, "weasal_amd", "csrc", "kpconv.hip")
PACKED = "kpconv_gather_bwd_x_packed_kernel"


def _hip_constant(name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(HIP).read())
    assert m, name
    return int(m.group(1))


def _variant(nq, ns, h, ci, dwf=0x10000000, dx=0x20000000, bf16=False, deformed=False, modulated=False, influence="linear",
             aggregation="sum", ordered=False):
    from weasal_amd import _lib, ops
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().ws_kpconv_gather_bwd_x_packed_variant(nq, ns, h, ci, dwf, dx, int(deformed), int(modulated), ops.INFLUENCE[influence],
                                                              ops.AGGREGATION[aggregation], int(bf16), int(ordered), buf, 256))
    return buf.value.decode()


def _group_ladder(ci):
    return 1 if ci <= 4 else 2 if ci <= 8 else 4 if ci <= 16 else 8 if ci <= 32 else 16


def test_reporter_names_the_packed_kernel_only_inside_its_scope():
    named = 0
    for ci in range(1, 301):
        for bf16 in (False, True):
            for off in (0, 1):
                es = 2 if bf16 else 4
                if bf16 and (ci % 4 or off):
                    continue                            # refused by every entry (rows_vec4_or_f32)
                for nq, ns in ((1000, 4000), (4000, 4000), (4001, 4000)):
                    for ordered in (False, True):
                        text = _variant(nq, ns, 40, ci, 0x10000000 + off * es, 0x20000000 + off * es, bf16=bf16, ordered=ordered)
                        if not bf16 and not off and ci % 4 == 0 and nq < ns:
                            assert text.startswith("%s<K=15, G=%d, VEC=true, T=float> grid=" % (PACKED, _group_ladder(ci))), (ci, text)
                            named += 1
                        else:
                            assert text == "none", (ci, bf16, off, nq, ns, text)
    assert named == 75 * 2
    # one operand off alignment is enough; every mode but rigid / linear / sum stays out
    assert _variant(1000, 4000, 40, 32, dwf=0x10000004) == "none" and _variant(1000, 4000, 40, 32, dx=0x20000004) == "none"
    for kw in (dict(deformed=True), dict(modulated=True), dict(influence="gaussian"), dict(influence="constant"), dict(aggregation="closest")):
        assert _variant(1000, 4000, 40, 32, **kw) == "none", kw


def test_mean_in_degree_boundary():
    pmax = _hip_constant("PACK_MEAN_MAX")
    assert 4 <= pmax <= 32                              # the range the sweep in profiles/ covers
    ns, h = 4000, 40
    for c in (pmax - 1, pmax):
        assert (c * ns) % h == 0
        nq = c * ns // h                                # nq * h == c * ns
        assert nq < ns and _variant(nq, ns, h, 32).startswith(PACKED), (c, nq)
    assert _variant(pmax * ns // h + 1, ns, h, 32) == "none"      # nq * h = PACK_MEAN_MAX * ns + h
    assert _variant(pmax * 400000 // 59, 400000, 59, 32).startswith(PACKED)
    assert _variant(pmax * 400000 // 59 + 1, 400000, 59, 32) == "none"


def test_grid_is_a_quad_per_wave():
    """four supports per wave, four waves per workgroup: ceil(ns / 16) workgroups up to the cap of the wave-per-item kernels"""
    for ns, grid in ((5, 1), (16, 1), (17, 2), (128, 8), (129, 16), (400000, 4096)):
        assert _variant(1, ns, 2, 32).endswith(" grid=%d" % grid), (ns, _variant(1, ns, 2, 32))
