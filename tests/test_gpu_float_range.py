"""Every query kernel against the oracle across the whole float range (tests/test_float_range.py establishes the oracle's own domain D on the
CPU; tests/float_range_cases.py holds the scenes, the scales 2^k and the admission table).

Per (scene, k) — every scene under 200 triangles, every batch under 1,000 rays, the oracle run to completion on exactly that input before
anything goes to the GPU:

  * closest hit through the 20 contexts of tests/test_gpu_edge_cases.py (host path and three device batches): for k in D the bars of that
    module unchanged (V8 family bit-exact against the oracle; the 4-wide kernels the oracle's closest hit up to ties and bit-exact against
    the exact model of their format); for k outside D the bit-exact bars through helpers.assert_same_bits_nan_aware — the number of
    NaN-excused fields must be the number the oracle (for a 4-wide kernel: its exact model) alone shows, 0 inside D; the 4-wide kernels
    keep the closest-hit bar against the oracle on every ray whose records are finite on both sides (its tie allowance compares distances).
    The compressed format refuses a scene exactly where
    racc_host_scene_wide_nodes refuses it;
  * occlusion == "the oracle reports a hit";
  * worlds two ways: an identity instance of the scaled scene, and the unscaled scene under 2^k I traced with the scaled rays (the
    kernel's own transform makes the extreme object-space ray), through world_helpers' composed expectation, intersect and occluded;
  * refit to vertices scaled by 2^k: the downloaded records equal racc_host_blobs_refit byte for byte (denormals are not flushed), then
    one trace against the oracle;
  * the admission table through every context, occluded, World.intersect and World.occluded."""
import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
import float_range_cases as frc
from float_range_cases import MISS, REJECTED, SCALES, SCENES
from helpers import (QUANT_VARIANTS, WIDE_FORMAT, WIDE_VARIANTS, assert_bit_exact, assert_same_bits_nan_aware, assert_same_closest_hit, assert_wide_exact, leaf_scene,
                     scale_geometry, wide_model)
from test_gpu_edge_cases import CONFIGS, ENV, _device_path, contexts      # noqa: F401 (contexts: the module-scoped fixture, instantiated for this module)
from world_helpers import IDENTITY, NO_INSTANCE

pytestmark = pytest.mark.gpu

CASES = [(name, k) for name in SCENES for k in SCALES]
REFIT_SCALES = (20, -20, 64, -64, 100, -100, -140)


def _case_id(c):
    return "%s, 2^%d" % c


@pytest.fixture(scope="module")
def plain():
    ctx = ra.Context(device=0)
    yield ctx
    ctx.destroy()


def _wide_or_refusal(blobs, fmt, rays, env):
    """The exact model's records for device format `fmt`, or the error code with which racc_host_scene_wide_nodes refuses the scene."""
    try:
        return wide_model(blobs, fmt, rays, env=env)[0]
    except ra.RaccError as e:
        return e.code


def _finite_records(a):
    hit = a["triangle"] != MISS
    return ~hit | (np.isfinite(a["t"]) & np.isfinite(a["u"]) & np.isfinite(a["v"]))


def run_range(contexts, blobs, rays, ref, what, exact, geometry, env=ENV, wide_against_oracle=True):
    """run_everywhere of tests/test_gpu_edge_cases.py with the oracle's records given (`ref`, computed before this call), the refusal of
    the compressed format and, for not `exact`, the NaN-aware comparison; there the 4-wide kernels keep the closest-hit bar against the
    oracle on every ray whose two records are finite (its tie allowance compares distances).  The reference's own kernel is not run here:
    it is built with fast-math and denormal flushing (oracle/Makefile), which is what these scales are about.
    -> {kernel family: NaN-excused fields per result array}."""
    model = {fmt: _wide_or_refusal(blobs, fmt, rays, env) for fmt in (45, 50)}
    assert not isinstance(model[45], int), "%s: the 128 B format refuses a scene (%s)" % (what, model[45])
    excused = {}
    for name, ctx in contexts.items():
        variant = CONFIGS[name].get("kernel_variant", 0)
        fmt = WIDE_FORMAT.get(variant)
        if fmt is not None and isinstance(model[fmt], int):
            with pytest.raises(ra.RaccError) as e:
                ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
            assert e.value.code == model[fmt], "%s | %s: upload refuses with %d, racc_host_scene_wide_nodes with %d" % (what, name, e.value.code, model[fmt])
            excused.setdefault("compressed, refused", set()).add(0)
            continue
        scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])      # (a refusal anywhere else raises here)
        e = ctx.create_environment(env)
        results = [("host path", ctx.intersect(scene, e, rays))] + [("device path, batch %d" % k, r) for k, r in enumerate(_device_path(ctx, scene, e, rays))]
        for path, got in results:
            label = "%s | %s | %s" % (what, name, path)
            if variant in WIDE_VARIANTS:
                family = "compressed" if variant in QUANT_VARIANTS else "4-wide"
                if wide_against_oracle:
                    sel = np.ones(len(rays), bool) if exact else (_finite_records(got) & _finite_records(ref))
                    arb = dict(geometry, rays=rays[sel]) if variant in QUANT_VARIANTS else None
                    assert_same_closest_hit(got[sel], ref[sel], label, max_ties=len(rays), arbiter=arb)
                if exact:
                    assert_wide_exact(got, model[fmt], label + " | exact model")
                    n = 0
                else:
                    n = assert_same_bits_nan_aware(got, model[fmt], label + " | exact model")
            else:
                family = "V8"
                if exact:
                    assert_bit_exact(got, ref, label)
                    n = 0
                else:
                    n = assert_same_bits_nan_aware(got, ref, label)
            excused.setdefault(family, set()).add(n)
        scene.destroy()
        e.destroy()
    return excused


# ------------------------------------------------------------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_closest_hit_on_every_scale(contexts, case):
    name, k = case
    c = frc.case(name, k)                                  # the oracle has run on exactly this input
    excused = run_range(contexts, c["blobs"], c["rays"], orc.traverse(c["blobs"], c["rays"], env=ENV), "%s, 2^%d" % case, c["in_domain"], c["geometry"])
    print("%s, 2^%d: %s, NaN-excused fields per result array %s (the oracle alone: %d)" % (name, k, "in D" if c["in_domain"] else "outside D", {f: sorted(n) for f, n in excused.items()}, c["nan_fields"]))
    # (assert_same_bits_nan_aware excuses exactly the oracle's NaN fields, so this restates its result: the count the issue asks to be shown)
    assert excused["V8"] == {c["nan_fields"]}, "the V8 family's NaN fields are not the oracle's"
    if c["in_domain"]:
        assert all(n == {0} for n in excused.values())


# -------------------------------------------------------------------------------------------------------------------------- occlusion
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_occlusion_on_every_scale(plain, case):
    name, k = case
    c = frc.case(name, k)
    want = (c["ref"]["triangle"] != MISS).astype(np.uint8)
    scene = plain.upload_scene(c["blobs"]["nodes"], c["blobs"]["pairs"], c["blobs"]["remap"])
    got = plain.occluded(scene, c["rays"])
    scene.destroy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s, 2^%d: occluded differs from the oracle at rays %s: got %s want %s" % (name, k, bad[:8], got[bad[:8]], want[bad[:8]])


# ----------------------------------------------------------------------------------------------------------------------------- worlds
def _assert_world(got, got_inst, want, want_inst, what):
    """world_helpers.assert_world_exact, a NaN field of the expectation only having to be a NaN.  -> the number of such fields."""
    assert np.array_equal(got_inst, want_inst), "%s: instance index differs at rays %s" % (what, np.nonzero(got_inst != want_inst)[0][:8])
    assert np.array_equal(got["triangle"], want["triangle"]), "%s: triangle differs at rays %s" % (what, np.nonzero(got["triangle"] != want["triangle"])[0][:8])
    excused = 0
    for f in ("t", "u", "v"):
        nan = np.isnan(want[f])
        excused += int(nan.sum())
        assert np.isnan(got[f][nan]).all(), "%s: %s holds a number where the expectation holds a NaN" % (what, f)
        bad = np.nonzero((got[f].view(np.uint32) != want[f].view(np.uint32)) & ~nan)[0]
        assert len(bad) == 0, "%s: %s not bit-exact at rays %s: got %r want %r" % (what, f, bad[:8], got[f][bad[:8]], want[f][bad[:8]])
    miss = want["triangle"] == MISS
    assert (want_inst[miss] == NO_INSTANCE).all() and (got["t"][miss] == 0).all()
    return excused


def _world_case(ctx, transform, blobs, rays, what):
    """One instance of `blobs` under `transform`: World.intersect and World.occluded against float_range_cases.world_expectation (the
    composed expectation behind the top-level rule).  Where the host preparation refuses the transform, create_world must refuse it with
    the same code.  -> (NaN-excused fields, composed hits the top level never enters) or None."""
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    try:
        exp, code = frc.world_expectation(transform, blobs, rays)      # the oracle, before anything is launched
        if exp is None:
            with pytest.raises(ra.RaccError) as e:
                ctx.create_world([(transform, scene)])
            assert e.value.code == code
            return None
        world = ctx.create_world([(transform, scene)])
        try:
            got, got_inst = world.intersect(rays)
            excused = _assert_world(got, got_inst, exp["want"], exp["want_inst"], what)
            occ = world.occluded(rays)
            assert np.array_equal(occ, exp["occluded"]), "%s: World.occluded differs at rays %s" % (what, np.nonzero(occ != exp["occluded"])[0][:8])
        finally:
            world.destroy()
        return excused, len(exp["culled_hits"])
    finally:
        scene.destroy()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_worlds_on_every_scale(plain, case):
    """An identity instance of the scaled scene, and the unscaled scene under 2^k I traced with the scaled rays, World.intersect and
    World.occluded.  Inside D: world_helpers' composed expectation, bit for bit, nothing culled, no NaN.  Outside D the composed
    expectation holds for every ray that enters the instance's padded world box by the top-level rule, and a miss for the others
    (tests/test_float_range.py shows on the CPU that the rule removes no hit inside D)."""
    name, k = case
    c = frc.case(name, k)
    blobs0, _, _ = frc.scene(name)
    a = _world_case(plain, IDENTITY, c["blobs"], c["rays"], "%s, 2^%d, identity instance of the scaled scene" % case)
    assert a is not None
    m = frc.scale_transform(k)
    b = _world_case(plain, m, blobs0, c["rays"], "%s, the unscaled scene under 2^%d I" % case) if m is not None else None
    print("%s, 2^%d: (NaN-excused fields, hits culled by the top level) %s (scaled scene), %s (scaled transform)" % (name, k, a, b))
    if c["in_domain"]:
        assert a == (0, 0) and b == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------------ refit
@pytest.mark.parametrize("k", REFIT_SCALES)
@pytest.mark.parametrize("name", ["leaf7 near_last", "soup, reference builder"])
def test_refit_to_scaled_vertices(plain, name, k):
    blobs0, geo0, rays0 = frc.scene(name)
    geo = scale_geometry(geo0, k)
    want = ra.host_refit(blobs0, geo["vertices"], geo["indices"])
    if k == -140:
        assert (np.abs(want["pairs"]["p0"][want["pairs"]["p0"] != 0]) < np.finfo(np.float32).tiny).all()      # every coordinate is a denormal
    rays = frc.case(name, k)["rays"]
    ref = orc.traverse(want, rays, env=ENV)
    scene = plain.upload_scene(blobs0["nodes"], blobs0["pairs"], blobs0["remap"])
    refit = plain.create_refit(scene, geo["indices"], len(geo["vertices"]))
    try:
        refit.refit(geo["vertices"])
        nodes, pairs = refit.download()
        assert nodes.tobytes() == np.ascontiguousarray(want["nodes"]).tobytes(), "%s, 2^%d: the refitted node records differ from racc_host_blobs_refit" % (name, k)
        assert pairs.tobytes() == np.ascontiguousarray(want["pairs"]).tobytes(), "%s, 2^%d: the refitted pair records differ from racc_host_blobs_refit" % (name, k)
        e = plain.create_environment(ENV)
        got = plain.intersect(scene, e, rays)
        e.destroy()
        n = assert_same_bits_nan_aware(got, ref, "%s refitted to 2^%d" % (name, k))
        assert n == int(sum(((ref["triangle"] != MISS) & np.isnan(ref[f])).sum() for f in ("t", "u", "v")))
    finally:
        refit.destroy()
        scene.destroy()


# -------------------------------------------------------------------------------------------------------------------- admission table
def test_admission_table_everywhere(contexts, plain):
    names, rays, expected = frc.admission_table()
    geo = frc.quad_geometry()
    blobs = orc.build_scene(geo["vertices"], geo["indices"])
    ref = orc.traverse(blobs, rays, env=ENV)
    assert not any(np.isnan(ref[f][ref["triangle"] != MISS]).any() for f in ("t", "u", "v"))
    for i, want in enumerate(expected):      # the hand-written outcomes hold for the oracle (tests/test_float_range.py) — and so for every kernel below
        if want == REJECTED:
            assert ref["triangle"][i] == MISS and ref["t"][i] == 0
        else:
            assert ref["triangle"][i] == want[1], names[i]
    excused = run_range(contexts, blobs, rays, ref, "admission table", True, geo)
    assert all(n == {0} for n in excused.values())
    scene = plain.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    occ = plain.occluded(scene, rays)
    bad = np.nonzero(occ != (ref["triangle"] != MISS))[0]
    assert len(bad) == 0, "occluded: rows %s" % [names[i] for i in bad]
    scene.destroy()
    n = _world_case(plain, IDENTITY, blobs, rays, "admission table, identity world")
    assert n == (0, 0)


# ----------------------------------------------------------------------------------------- known answers that tell injected faults apart
def test_nan_plane_minnum_everywhere(contexts, plain):
    """float_range_cases.nan_plane_case: a NaN as the second operand of the slab test's min / max.  The oracle (minNum) misses, by hand; the
    V8 family must agree bit for bit — with the select a < b ? a : b the oracle reported triangle 0.  The 4-wide kernels evaluate the slab
    as (plane - o) / d, which makes no NaN here: they answer to their exact model alone.  The compressed format refuses the infinite plane
    exactly as racc_host_scene_wide_nodes does.  Occlusion as the oracle."""
    for infinite in (False, True):
        blobs, rays, want = frc.nan_plane_case(infinite)
        ref = orc.traverse(blobs, rays, env=ENV)
        assert ref["triangle"][0] == want
        excused = run_range(contexts, blobs, rays, ref, "NaN plane (infinite: %s)" % infinite, True, None, wide_against_oracle=False)
        assert ("compressed, refused" in excused) == infinite and all(n == {0} for n in excused.values())
        scene = plain.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
        assert np.array_equal(plain.occluded(scene, rays), (ref["triangle"] != MISS).astype(np.uint8))
        scene.destroy()


def test_exact_tie_inside_a_pair_everywhere(contexts, plain):
    """float_range_cases.tie_pair_case: both triangles of the pair accept at equal T |det|; the strict pick keeps the first, in every kernel."""
    blobs, rays, want = frc.tie_pair_case()
    ref = orc.traverse(blobs, rays, env=ENV)
    assert np.array_equal(ref["triangle"], want)
    excused = run_range(contexts, blobs, rays, ref, "exact tie inside a pair", True, frc.geometry_of_blobs(blobs))
    assert all(n == {0} for n in excused.values())
