"""Occlusion queries on worlds (racc_hip_world_occluded_device) against the world closest-hit path on the same rays, in the same session.

   The three worlds of tools/bench_world.py: one identity instance of battlefield-synth (the library's default tree), and N = 64 and
   N = 4,096 instances of a small mesh (battlefield-synth at grid=40, boxes=32, quads=100: 3,784 triangles) on a square grid.  1M shadow
   rays per world, made as tools/bench_occlusion.py makes them: from the hit points of the world's own 1024x1024 primary batch toward one
   fixed sun direction, origins moved 1e-3 along the ray, maxT = 1e6.
   Timed: K launches between two synchronisations after a warm-up round, the paths in turn, ROUNDS times over; Mrays/s as median with min
   and max of the rounds.  Paths: World.occluded_device (the new query), World.intersect_device on the same rays (the baseline: code this
   query does not touch) and, for the identity world only, Context.occluded_device on the plain scene.  Per world: the ratio to the
   baseline, the baseline's min-max spread, whether the occlusion median beats the baseline's by more than that spread, and the occluded
   fraction; occlusion and closest hit are checked to agree on every ray.  Prints one JSON line.

   python tools/bench_world_occlusion.py [--rounds 5] [--k 10] [--sizes 64,4096]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth

SUN = np.array([0.35, 0.8, 0.48])
COUNT = 1 << 20
IDENTITY = np.eye(3, 4, dtype=np.float32)


def shadow_rays(world, camera):
    prim, _ = synth.primary_rays(camera, 1024, 1024)
    hits, inst = world.intersect(prim)
    hit = np.nonzero(inst != ra.NO_INSTANCE)[0]
    hit = np.resize(hit, COUNT)      # misses are skipped, the hit list is re-cycled until COUNT rays exist (as tools/bench_occlusion.py does)
    sun = SUN / np.linalg.norm(SUN)
    p = prim["origin"][hit].astype(np.float64) + prim["dir"][hit].astype(np.float64) * hits["t"][hit].astype(np.float64)[:, None]
    rays = np.zeros(COUNT, synth.RAY_DTYPE)
    rays["origin"] = (p + 1e-3 * sun).astype(np.float32)
    rays["dir"] = sun.astype(np.float32)
    rays["minT"], rays["maxT"] = 0.0, 1e6
    return rays


def measure(ctx, runs, rounds, k):
    rates = {name: [] for name in runs}
    for rnd in range(rounds + 1):      # round 0 is the warm-up
        for name, go in runs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            go()
            dt = time.perf_counter() - t0
            if rnd:
                rates[name].append(k * COUNT / dt / 1e6)
    return {name: dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1)) for name, v in rates.items()}


def compare(ctx, world, camera, k, rounds, plain_scene=None):
    """The paths over one device-resident batch of shadow rays; returns the world's entry of the JSON line."""
    rays = shadow_rays(world, camera)
    d_rays = ctx.alloc(rays.nbytes); d_rays.upload(rays)
    st = ctx.create_stream()
    d_occ, d_plain, d_res, d_inst = ctx.alloc(COUNT), ctx.alloc(COUNT), ctx.alloc(COUNT * 16), ctx.alloc(COUNT * 4)

    def run_occluded():
        for _ in range(k):
            world.occluded_device(d_rays.ptr, d_occ.ptr, COUNT, stream=st)
        ctx.stream_synchronize(st)

    def run_closest():
        for _ in range(k):
            world.intersect_device(d_rays.ptr, d_res.ptr, d_inst.ptr, COUNT, stream=st)
        ctx.stream_synchronize(st)

    def run_plain():
        for _ in range(k):
            ctx.occluded_device(plain_scene, d_rays.ptr, d_plain.ptr, COUNT, stream=st)
        ctx.stream_synchronize(st)

    runs = {"world_occluded": run_occluded, "world_closest_hit": run_closest}
    if plain_scene is not None:
        runs["scene_occluded"] = run_plain
    stat = measure(ctx, runs, rounds, k)
    occ = d_occ.download(np.uint8, COUNT)
    assert np.array_equal(occ, (d_inst.download(np.uint32, COUNT) != ra.NO_INSTANCE).astype(np.uint8)), "world occlusion and world closest hit disagree"
    if plain_scene is not None:
        assert np.array_equal(occ, d_plain.download(np.uint8, COUNT)), "world occlusion and scene occlusion disagree on the identity world"
    for b in (d_rays, d_occ, d_plain, d_res, d_inst):
        b.free()
    ctx.destroy_stream(st)
    base = stat["world_closest_hit"]
    return dict(mrays_per_s=stat, baseline="world_closest_hit", ratio=round(stat["world_occluded"]["median"] / base["median"], 3),
                baseline_spread=[base["min"], base["max"]], occluded_fraction=round(float(occ.mean()), 4),
                beats_baseline_by_more_than_its_spread=bool(stat["world_occluded"]["median"] - base["median"] > base["max"] - base["min"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", default="64,4096")
    args = ap.parse_args()
    ctx = ra.Context(device=0)
    out = dict(tool="bench_world_occlusion", rays=COUNT, k=args.k, rounds=args.rounds)

    # one identity instance of battlefield-synth
    sc = synth.battlefield_synth()
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=None)
    scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
    world = ctx.create_world([(IDENTITY, scene)])
    out["one_identity_instance"] = dict(scene=sc["name"], **compare(ctx, world, sc["camera"], args.k, args.rounds, plain_scene=scene))
    world.destroy(); scene.destroy()

    # N instances of a small mesh on a square grid (placement and camera as tools/bench_world.py)
    mesh = synth.battlefield_synth(grid=40, boxes=32, quads=100)
    mesh_host = ra.HostScene(mesh["vertices"], mesh["indices"], quality=None)
    mesh_scene = ctx.upload_scene(mesh_host.nodes, mesh_host.pairs, mesh_host.remap)
    pitch = 200.0
    out["instances"] = {}
    for n in [int(s) for s in args.sizes.split(",")]:
        side = int(round(np.sqrt(n)))
        assert side * side == n
        transforms = np.tile(IDENTITY, (n, 1, 1))
        transforms[:, 0, 3] = pitch * (np.arange(n) % side); transforms[:, 2, 3] = pitch * (np.arange(n) // side)
        world = ctx.create_world([(m, mesh_scene) for m in transforms])
        w = pitch * side
        camera = dict(mesh["camera"], origin=np.array([0.5 * w - 100.0, 0.35 * w + 60.0, -0.25 * w - 100.0], np.float32),
                      target=np.array([0.5 * w - 100.0, 0.0, 0.4 * w - 100.0], np.float32))
        out["instances"][str(n)] = dict(triangles=int(n * len(mesh["indices"])), **compare(ctx, world, camera, args.k, args.rounds))
        world.destroy()
    mesh_scene.destroy()
    print(json.dumps(out), flush=True)
    ctx.destroy()


if __name__ == "__main__":
    main()
