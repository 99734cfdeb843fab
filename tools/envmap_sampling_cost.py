#!/usr/bin/env python3
"""What a refresh of the environment map's importance-sampling tables costs, and what it buys.

  cost   the host's build_tables (zdr_amd/envmap.py) timed once, beside the rebuild on the device (zdr_scene_update_envmap_sampling) with
         compensate_mis on and off and one forward + backward with envmap= of the environment-only scene at 512^2 spp 64.  Same
         process, same box; the three device sides ALTERNATE round by round, each round is `--reps` calls between two device events,
         and the median, minimum and maximum over the rounds are reported.
  gain   the stale-table case of tests/test_gpu_envmap_sampling.py: tables of map A (the sun upper left), the map replaced by B (the sun
         upper right), 64^2 spp 4 against spp 1024: RMSE with A's tables and after the rebuild.  With --oracle the same on the CPU, from the
         oracle and the host's tables.

    python tools/envmap_sampling_cost.py [--sky 256] [--rounds 7] [--reps 10] [--warmup 3] [--oracle] [--out profiles/envmap_sampling_cost.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import envmap_tables as T  # noqa: E402
from zdr_amd import envmap as E  # noqa: E402
from zdr_amd.scenes import CBOX_CAMERA, cbox_models, fd_material_np  # noqa: E402
from envgrad_cost import sun_sky  # noqa: E402


def window(fn, reps):
    """ms per call of `reps` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def rmse(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))


def gain_gpu(integrator):
    A, B = T.sun_map((32, 64), T.SUN_A), T.sun_map((32, 64), T.SUN_B)
    scene = T.set_map_with_uniform_tables(T.env_only_scene(integrator), A)
    m = torch.from_numpy(fd_material_np(64, 0)).cuda()
    scene.update_envmap_sampling(None, on_device=True)
    scene.set_envmap_texture(torch.from_numpy(E.prepare_image(B)).cuda())
    stale = [scene.render_forward(m, (64, 64), 4, seed)[..., :3].cpu().numpy() for seed in (1, 2, 3)]
    scene.update_envmap_sampling(None, on_device=True)
    fresh = [scene.render_forward(m, (64, 64), 4, seed)[..., :3].cpu().numpy() for seed in (1, 2, 3)]
    ref = scene.render_forward(m, (64, 64), 1024, 100)[..., :3].cpu().numpy()
    return [(rmse(s, ref), rmse(f, ref)) for s, f in zip(stale, fresh)]


def gain_oracle(integrator):
    import oracle
    from zdr_amd import geometry
    A, B = T.sun_map((32, 64), T.SUN_A), T.sun_map((32, 64), T.SUN_B)
    IB, TA, TB = E.prepare_image(B), T.host_tables(A), T.host_tables(B)
    S = oracle.OracleScene.from_arrays(geometry.assemble([(cbox_models()[0][0], None, 0.0)]))
    mat = fd_material_np(64, 0)

    def render(tables, spp, seed):
        S.set_envmap(IB, *tables)
        return S.render_forward(oracle.make_params(integrator, 64, 64, spp, seed, CBOX_CAMERA, mat.shape[:2]), mat)[..., :3]

    ref = render(TB, 1024, 100)
    return [(rmse(render(TA, 4, seed), ref), rmse(render(TB, 4, seed), ref)) for seed in (1, 2, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sky", type=int, default=256, help="height of the 1:2 map (its square form is 2h x 2h)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle", action="store_true", help="the stale-table case on the CPU as well (oracle + host tables, about a minute)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sky = sun_sky(args.sky)
    I = E.prepare_image(sky)
    t0 = time.perf_counter()
    E.build_tables(I)
    host_s = time.perf_counter() - t0

    scene = T.set_map_with_uniform_tables(T.env_only_scene("path"), sky)
    m = torch.from_numpy(fd_material_np(128, 1)).cuda().requires_grad_()
    env = torch.from_numpy(sky).cuda().requires_grad_()
    W, spp = 512, 64

    def rebuild_on():
        scene.update_envmap_sampling(None, compensate_mis=True, on_device=True)

    def rebuild_off():
        scene.update_envmap_sampling(None, compensate_mis=False, on_device=True)

    def step():
        m.grad = env.grad = None
        scene.render(m, res=(W, W), spp=spp, seed=0, envmap=env).sum().backward()

    for _ in range(args.warmup):
        rebuild_off(); rebuild_on(); step()
    t = {"rebuild_compensated": [], "rebuild_plain": [], "forward_backward_env": []}
    for _ in range(args.rounds):
        t["rebuild_compensated"].append(window(rebuild_on, args.reps)); t["rebuild_plain"].append(window(rebuild_off, args.reps))
        rebuild_on()
        t["forward_backward_env"].append(window(step, args.reps))
    scene.check()
    T.check_tables(*scene.envmap_sampling_tables(), bar=T.Q_BAR)
    out = {k: stats(v) for k, v in t.items()}
    out["host_build_tables_s"] = host_s
    out["rebuild_over_step"] = out["rebuild_compensated"]["median_ms"] / out["forward_backward_env"]["median_ms"]
    fmt = lambda s: f"{s['median_ms']:8.3f} ms [{s['min_ms']:.3f}, {s['max_ms']:.3f}]"  # noqa: E731
    lines = [f"{args.sky} x {2 * args.sky} map: host build_tables {host_s:6.2f} s (once)   device rebuild, compensate_mis on {fmt(out['rebuild_compensated'])}  off {fmt(out['rebuild_plain'])}",
             f"environment-only scene {W}^2 spp {spp}, forward + backward with envmap= {fmt(out['forward_backward_env'])}   rebuild / step = {out['rebuild_over_step']:.4f}"
             f"   host / device = {host_s * 1e3 / out['rebuild_compensated']['median_ms']:.0f} x"]
    out["gain"] = {}
    for integrator in ("path", "direct"):
        sides = [("MI355X, device tables", gain_gpu(integrator))] + ([("CPU oracle, host tables", gain_oracle(integrator))] if args.oracle else [])
        for side, g in sides:
            out["gain"][f"{integrator} / {side}"] = g
            lines.append(f"stale tables -> after the rebuild, {integrator} 64^2 spp 4 RMSE against spp 1024, seeds 1-3 ({side}): "
                         + "  ".join(f"{s:.4g} -> {f:.4g} ({f / s:.3f})" for s, f in g))
    print("\n".join(lines))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/envmap_sampling_cost.py --sky {args.sky} --rounds {args.rounds} --reps {args.reps}{' --oracle' if args.oracle else ''} on {torch.cuda.get_device_name(0)}\n"
                    + "\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
