"""Refit of a world's top level on the device against the rebuild, in one session.

   N = 2^10, 2^16 and 2^20 instances of one small mesh (battlefield-synth at grid=40, boxes=32, quads=100: 3,784 triangles) on a square
   grid.  The new transforms permute the instances among their grid positions (a fixed random permutation): every instance moves, the set
   of positions stays — the worst case for kept topology.  Reports, as one JSON line, per N:
     1. refit_device_ms   one racc_hip_world_refit_device with device-resident transforms: HIP events on the stream around the call,
                          median of 20 after 3 warm-ups, with min and max
     2. update_ms         racc_hip_world_update for the same transforms (wall clock, median of 3): the blocking rebuild, the baseline
     3. trace             Mrays/s of racc_hip_world_intersect_device over a 1M-ray primary batch (K launches between two
                          synchronisations, median of the rounds) on the REFITTED tree against the REBUILT tree for the same transforms,
                          and whether both report the same records: the cost of kept topology.  A random permutation leaves the old
                          tree's boxes covering the whole grid, so a ray on the refitted tree enters a large part of all instances: it
                          is traced with every 16th ray of the batch (65,536 incoherent rays: not the rebuilt tree's conditions), ONE launch per
                          round and two rounds — at 2^20 instances one launch of the full batch takes minutes
   No ratio here is asserted anywhere; DESIGN.md quotes a run.

   python tools/bench_world_refit.py [--sizes 1024,65536,1048576] [--rounds 5] [--k 10]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth

COUNT = 1 << 20
IDENTITY = np.eye(3, 4, dtype=np.float32)


def hip_runtime():
    """The HIP runtime the engine is linked against (for events on the refit's stream)."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def stats(xs, digits=4):
    return dict(median=round(float(np.median(xs)), digits), min=round(float(np.min(xs)), digits), max=round(float(np.max(xs)), digits))


SPARSE = COUNT // 16      # the rays the refitted tree is traced with


def mrays(ctx, world, d_rays, d_res, d_inst, st, count, k, rounds):
    rates = []
    for rnd in range(rounds + 1):      # round 0 is the warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            world.intersect_device(d_rays.ptr, d_res.ptr, d_inst.ptr, count, stream=st)
        ctx.stream_synchronize(st)
        if rnd:
            rates.append(k * count / (time.perf_counter() - t0) / 1e6)
    return stats(rates, 3), d_res.download(synth.RESULT_DTYPE, count), d_inst.download(np.uint32, count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    hip = hip_runtime()
    mesh = synth.battlefield_synth(grid=40, boxes=32, quads=100)
    pitch = 200.0
    out = dict(tool="bench_world_refit", rays=COUNT, k=args.k, rounds=args.rounds, instances={})
    with ra.Context(device=0) as ctx:
        host = ra.HostScene(mesh["vertices"], mesh["indices"], quality=None)
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        st = ctx.create_stream()
        d_rays, d_res, d_inst, d_sparse = ctx.alloc(COUNT * 32), ctx.alloc(COUNT * 16), ctx.alloc(COUNT * 4), ctx.alloc(SPARSE * 32)
        e0, e1 = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
        for n in [int(s) for s in args.sizes.split(",")]:
            side = int(round(np.sqrt(n)))
            assert side * side == n
            built = np.tile(IDENTITY, (n, 1, 1))
            built[:, 0, 3] = pitch * (np.arange(n) % side); built[:, 2, 3] = pitch * (np.arange(n) // side)
            moved = np.ascontiguousarray(built[np.random.RandomState(n).permutation(n)])
            w = pitch * side
            camera = dict(mesh["camera"], origin=np.array([0.5 * w - 100.0, 0.35 * w + 60.0, -0.25 * w - 100.0], np.float32),
                          target=np.array([0.5 * w - 100.0, 0.0, 0.4 * w - 100.0], np.float32))
            prim, _ = synth.primary_rays(camera, 1024, 1024)
            d_rays.upload(prim)
            d_sparse.upload(np.ascontiguousarray(prim[::16]))
            world = ctx.create_world([(m, scene) for m in built])
            handle = world.create_refit()
            d_t = ctx.alloc(moved.nbytes)
            d_t.upload(moved.reshape(n, 12))

            # 1. one device refit
            ms = []
            for i in range(23):
                hip.hipEventRecord(e0, st)
                handle.refit_device(d_t.ptr, stream=st)
                hip.hipEventRecord(e1, st)
                ctx.stream_synchronize(st)
                t = C.c_float(0)
                hip.hipEventElapsedTime(C.byref(t), e0, e1)
                if i >= 3:
                    ms.append(t.value)
            row = dict(refit_device_ms=stats(ms), disabled=handle.check())
            got = world.download()
            rb = np.tile(ra.root_box(host.nodes), (n, 1))
            row["inv_equals_host_prepare"] = bool(got["inv"].tobytes() == ra.host_world_prepare(moved, rb)["inv"].tobytes())

            # 3a. the refitted tree
            row["refitted_mrays_per_s"], res_a, inst_a = mrays(ctx, world, d_sparse, d_res, d_inst, st, SPARSE, 1, 2)

            # 2. the blocking rebuild for the same transforms (it also rebuilds the handle's tables), 3b. the rebuilt tree
            ups = []
            for _ in range(3):
                t0 = time.perf_counter()
                world.update(moved)
                ups.append((time.perf_counter() - t0) * 1e3)
            row["update_ms"] = stats(ups, 3)
            row["rebuilt_mrays_per_s"], res_b, inst_b = mrays(ctx, world, d_rays, d_res, d_inst, st, COUNT, args.k, args.rounds)
            row["refit_over_update"] = round(row["refit_device_ms"]["median"] / row["update_ms"]["median"], 6)
            row["refitted_over_rebuilt"] = round(row["refitted_mrays_per_s"]["median"] / row["rebuilt_mrays_per_s"]["median"], 6)
            row["same_records"] = bool(res_a.tobytes() == res_b[::16].tobytes() and inst_a.tobytes() == inst_b[::16].tobytes())
            row["hit_fraction"] = round(float((inst_b != ra.NO_INSTANCE).mean()), 4)
            row["world_info"] = world.info
            out["instances"][str(n)] = row
            print(json.dumps({str(n): row}), file=sys.stderr, flush=True)
            handle.destroy(); world.destroy(); d_t.free()
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
        for b in (d_rays, d_res, d_inst, d_sparse):
            b.free()
        ctx.destroy_stream(st)
        scene.destroy()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
