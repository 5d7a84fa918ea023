"""Occlusion queries against the closest-hit path on the same rays, in the same session.

   battlefield-synth, the library's default tree.  1M shadow rays: from the first-bounce hit points of the 1024x1024 primary batch (the
   engine's own hits) toward one fixed sun direction, origins moved 1e-3 along the ray, maxT = 1e6.  Timed: K = 20 launches between two
   synchronisations, after a warm-up — racc_hip_occluded_device over three streams in rotation, racc_hip_intersect_device (no probe image,
   LANE_AUTO) on a chain_launches=2 context and on a default context.  The three are measured in turn, ROUNDS times over.  Prints one JSON
   line: Mrays/s of each (median of the rounds, with min and max), the ratio to the faster baseline, the occluded fraction, that
   baseline's min-max spread, and whether the occlusion median beats that baseline's by more than the spread.

   python tools/bench_occlusion.py [--rounds 7] [--k 20] [--streams 3]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth

SUN = np.array([0.35, 0.8, 0.48])
COUNT = 1 << 20


def shadow_rays(ctx, scene, sc):
    prim, _ = synth.primary_rays(sc["camera"], 1024, 1024)
    hits = ctx.intersect(scene, None, prim)
    hit = np.nonzero(hits["triangle"] != synth.INVALID_TRIANGLE)[0]
    hit = np.resize(hit, COUNT)      # misses are skipped, the hit list is re-cycled until COUNT rays exist (as synth.diffuse_bounce_rays does)
    sun = SUN / np.linalg.norm(SUN)
    p = prim["origin"][hit].astype(np.float64) + prim["dir"][hit].astype(np.float64) * hits["t"][hit].astype(np.float64)[:, None]
    rays = np.zeros(COUNT, synth.RAY_DTYPE)
    rays["origin"] = (p + 1e-3 * sun).astype(np.float32)
    rays["dir"] = sun.astype(np.float32)
    rays["minT"], rays["maxT"] = 0.0, 1e6
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--streams", type=int, default=3)
    args = ap.parse_args()
    assert args.rounds >= 5
    sc = synth.battlefield_synth()
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=None)
    ctxs = {"default": ra.Context(device=0), "chain_launches=2": ra.Context(device=0, chain_launches=2)}
    scenes = {k: c.upload_scene(host.nodes, host.pairs, host.remap) for k, c in ctxs.items()}
    rays = shadow_rays(ctxs["default"], scenes["default"], sc)
    dev = {}
    for k, c in ctxs.items():
        d_r = c.alloc(rays.nbytes); d_r.upload(rays)
        dev[k] = dict(rays=d_r, hits=[c.alloc(COUNT * 16) for _ in range(3)])
    ctx = ctxs["default"]
    streams = [ctx.create_stream() for _ in range(args.streams)]
    d_occ = [ctx.alloc(COUNT) for _ in streams]

    def run_occlusion():
        for i in range(args.k):
            ctx.occluded_device(scenes["default"], dev["default"]["rays"].ptr, d_occ[i % len(streams)].ptr, COUNT, stream=streams[i % len(streams)])
        for s in streams:
            ctx.stream_synchronize(s)

    def run_closest(name):
        def go():
            for i in range(args.k):
                ctxs[name].intersect_device(scenes[name], None, dev[name]["rays"].ptr, dev[name]["hits"][i % 3].ptr, COUNT, lane=ra.LANE_AUTO)
            ctxs[name].wait(ra.LANE_AUTO)
        return go

    runs = {"occluded": run_occlusion, "closest_hit_chain_launches_2": run_closest("chain_launches=2"), "closest_hit_default": run_closest("default")}
    rates = {k: [] for k in runs}
    for rnd in range(args.rounds + 1):      # round 0 is the warm-up
        for name, go in runs.items():
            for c in ctxs.values():
                c.synchronize()
            t0 = time.perf_counter()
            go()
            dt = time.perf_counter() - t0
            if rnd:
                rates[name].append(args.k * COUNT / dt / 1e6)
    occ = d_occ[0].download(np.uint8, COUNT)
    closest = dev["default"]["hits"][0].download(synth.RESULT_DTYPE, COUNT)
    assert np.array_equal(occ, (closest["triangle"] != synth.INVALID_TRIANGLE).astype(np.uint8)), "occlusion and closest hit disagree"
    stat = {k: dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1)) for k, v in rates.items()}
    base = max(("closest_hit_chain_launches_2", "closest_hit_default"), key=lambda k: stat[k]["median"])
    print(json.dumps(dict(tool="bench_occlusion", scene=sc["name"], rays=COUNT, k=args.k, rounds=args.rounds, streams=args.streams, mrays_per_s=stat,
                          baseline=base, ratio=round(stat["occluded"]["median"] / stat[base]["median"], 3),
                          baseline_spread=[stat[base]["min"], stat[base]["max"]], occluded_fraction=round(float(occ.mean()), 4),
                          beats_baseline_by_more_than_its_spread=bool(stat["occluded"]["median"] - stat[base]["median"] > stat[base]["max"] - stat[base]["min"]))), flush=True)
    for s in streams:
        ctx.destroy_stream(s)
    for c in ctxs.values():
        c.destroy()


if __name__ == "__main__":
    main()
