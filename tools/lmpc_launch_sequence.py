"""The launch sequence of the LMPC closed-loop entries, for comparing two builds of the library kernel by kernel.

`run` makes, with the restoration phases on and then off, one rollout_dev, one collect_dev and one train_global_dev
call of two iterations at B = 2, N = 4, steps = 4 (record_every = 2, a reset pool of one row; the global buffer
starts one draw short of full, so the first iteration runs the global update), all on the handle's stream; then, on
a second handle, one train_pop_global_dev call of the same shape for P = 2 learners (their buffers one draw short of
full as well).  Under a kernel trace (run alone, the program after `--`):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/lmpc_launch_sequence.py run
    python tools/lmpc_launch_sequence.py list <dir> profiles/abi_split/launch_sequence_<build>.txt

`list` writes, per stream (queue when the trace has no stream column), one line per dispatch in dispatch order: kernel
name, grid and workgroup sizes.  Two builds launch the same sequence exactly when the two files are equal; an A/B
build of another commit is selected with DART_MPC_AB=1 DART_MPC_LIB=<its library in the package directory>.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))

B, N, STEPS, EVERY, EPOCHS, MB, ITERATIONS, P = 2, 4, 4, 2, 1, 4, 2, 2


def run():
    import numpy as np
    import torch
    from dart_mpc import _lib, ppo
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch

    D = lmpc_batch(1)
    up = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    ptr = lambda d: {k: v.data_ptr() for k, v in d.items()}
    R = STEPS // EVERY
    n = R * B
    m, G = _lib.global_rows(n)
    for restoration in (True, False):
        s = _lib.LmpcSolver(N=N, B_max=B, restoration=restoration)
        rng = np.random.default_rng(3)
        pol = LmpcPolicy(B, seed=0, critic_weights=0.05 * rng.standard_normal(_lib.CRITIC_NWEIGHTS).astype(np.float32))
        c = up(dict(target=D["target"][:B], prm=np.tile(_lib.LMPC_PRM_DEFAULT, (B, 1)), pvec=D["pvec"][:B],
                    current_k=pol.current_k, weights=pol.weights, critic=pol.critic_weights,
                    noise=rng.standard_normal((STEPS, B, 34)).astype(np.float32)))
        st = up(s.loop_state(D["state"][:B], policy=pol))
        cs = up(s.collect_state(np.zeros((B, 2))))
        pool = up({"reset_x": D["state"][None, B:2 * B], "reset_target": D["target"][None, B:2 * B],
                   "reset_pvec": D["pvec"][None, B:2 * B]})
        lg, clg = up(_lib.loop_logs(_lib.LMPC_LOOP_LOGS, STEPS, B)), up(_lib.loop_logs(_lib.LMPC_COLLECT_LOGS, STEPS, B))
        rec = up(_lib.loop_logs(_lib.LMPC_COLLECT_REC, R, B))
        pcfg, rcfg = pol.cfg, _lib.reward_config(record_every=EVERY, max_episode_steps=3)
        tr = up(dict(adam=np.zeros((2, _lib.PPO_NPARAMS), np.float32), adam_step=np.zeros(1, np.int32),
                     train_log=np.zeros((ITERATIONS, _lib.TRAIN_LOG_COLS)), best_return=np.full(1, -np.inf),
                     best_weights=np.zeros(_lib.PPO_NPARAMS, np.float32), best_iter=np.zeros(1, np.int32)))
        tr["workspace"] = torch.zeros(_lib.train_workspace_bytes(B, STEPS, EVERY, EPOCHS, MB), dtype=torch.uint8,
                                      device="cuda")
        gb = {f: torch.zeros((G, w) if w else (G,), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
              for f, w, dt in _lib.LMPC_GLOBAL_ARRAYS}
        glog = torch.zeros(ITERATIONS, _lib.GLOBAL_LOG_COLS, dtype=torch.float64, device="cuda")
        gws = torch.zeros(_lib.global_workspace_bytes(n, EPOCHS, MB), dtype=torch.uint8, device="cuda")
        g = _lib.global_buffer(ptr(gb), G, n - m, global_log=glog.data_ptr(), workspace=gws.data_ptr())
        torch.cuda.synchronize()        # (every fill kernel of the allocations above ahead of the library's launches)
        cp = (c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr())
        s.rollout_dev(B, 0, STEPS, STEPS, *cp, ptr(st), ptr(lg), pcfg=pcfg, weights=c["weights"].data_ptr(),
                      current_k=c["current_k"].data_ptr(), noise=c["noise"].data_ptr())
        s.collect_dev(B, 0, STEPS, STEPS, R, 1, *cp, ptr(st), ptr(cs), ptr(lg), ptr(clg), ptr(rec), pcfg, rcfg,
                      c["weights"].data_ptr(), c["critic"].data_ptr(), c["current_k"].data_ptr(),
                      noise=c["noise"].data_ptr(), pool=ptr(pool))
        tcfg = _lib.train_config(seed=5, iterations=ITERATIONS, steps=STEPS)
        s.train_global_dev(B, 1, *cp, c["current_k"].data_ptr(), c["weights"].data_ptr(), c["critic"].data_ptr(),
                           ptr(st), ptr(cs), ptr(lg), ptr(clg), ptr(rec), ptr(tr), pcfg, rcfg,
                           _lib.ppo_config(epochs=EPOCHS, mini_batch_size=MB), tcfg, g, pool=ptr(pool))
        s.sync()
        torch.cuda.synchronize()
        print(f"restoration {int(restoration)}: library {_lib.LIB_NAME}, train_log n = "
              f"{tr['train_log'].cpu().numpy()[:, 0].tolist()}, global fill = {glog.cpu().numpy()[:, 0].tolist()}",
              flush=True)
        s.close()
        # the population's form of the same call: P learners of B instances, stacked learner-major
        NI = P * B
        s = _lib.LmpcSolver(N=N, B_max=NI, restoration=restoration)
        pol = LmpcPolicy(NI, seed=0, critic_weights=pol.critic_weights)
        c = up(dict(target=D["target"][:NI], prm=np.tile(_lib.LMPC_PRM_DEFAULT, (NI, 1)), pvec=D["pvec"][:NI],
                    current_k=pol.current_k, weights=np.stack([pol.weights] * P),
                    critic=ppo.stack_critics([pol.critic_weights] * P)))
        st = up(s.loop_state(D["state"][:NI], policy=pol))
        cs = up(s.collect_state(np.zeros((NI, 2))))
        pool = up({"reset_x": D["state"][None, NI:2 * NI], "reset_target": D["target"][None, NI:2 * NI],
                   "reset_pvec": D["pvec"][None, NI:2 * NI]})
        lg, clg = up(_lib.loop_logs(_lib.LMPC_LOOP_LOGS, STEPS, NI)), up(_lib.loop_logs(_lib.LMPC_COLLECT_LOGS, STEPS, NI))
        rec = up(_lib.loop_logs(_lib.LMPC_COLLECT_REC, R, NI))
        tr = up(dict(adam=np.zeros((P, 2, _lib.PPO_NPARAMS), np.float32), adam_step=np.zeros(P, np.int32),
                     train_log=np.zeros((P, ITERATIONS, _lib.TRAIN_LOG_COLS)), best_return=np.full(P, -np.inf),
                     best_weights=np.zeros((P, _lib.PPO_NPARAMS), np.float32), best_iter=np.zeros(P, np.int32)))
        tr["workspace"] = torch.zeros(_lib.train_pop_workspace_bytes(P, B, STEPS, EVERY, EPOCHS, MB), dtype=torch.uint8,
                                      device="cuda")
        gb = {f: torch.zeros((P, G, w) if w else (P, G), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
              for f, w, dt in _lib.LMPC_GLOBAL_ARRAYS}
        glog = torch.zeros(P, ITERATIONS, _lib.GLOBAL_LOG_COLS, dtype=torch.float64, device="cuda")
        gws = torch.zeros(_lib.global_pop_workspace_bytes(P, n, G, EPOCHS, MB), dtype=torch.uint8, device="cuda")
        g = _lib.global_buffer(ptr(gb), G, n - m, global_log=glog.data_ptr(), workspace=gws.data_ptr())
        torch.cuda.synchronize()
        s.train_pop_global_dev(P, [5, 6], B, 1, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(),
                               c["current_k"].data_ptr(), c["weights"].data_ptr(), c["critic"].data_ptr(), ptr(st),
                               ptr(cs), ptr(lg), ptr(clg), ptr(rec), ptr(tr), pol.cfg, rcfg,
                               _lib.ppo_config(epochs=EPOCHS, mini_batch_size=MB), tcfg, g, pool=ptr(pool))
        s.sync()
        torch.cuda.synchronize()
        print(f"restoration {int(restoration)}: population of {P}, train_log n = "
              f"{tr['train_log'].cpu().numpy()[:, :, 0].tolist()}, global fill = {glog.cpu().numpy()[:, :, 0].tolist()}",
              flush=True)
        s.close()


def listing(src, dst):
    traces = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        raise SystemExit(f"no *kernel_trace.csv under {src}")
    rows = []
    for path in traces:
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    # per stream (queue when the trace has no stream column), the streams numbered by first use
    key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
    per = {}
    for r in rows:
        per.setdefault(r[key], []).append(r)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        for i, rs in enumerate(per.values()):
            fh.write(f"# {key[:-3].lower()} {i}: {len(rs)} dispatches\n")
            for r in rs:
                fh.write(f"{r['Kernel_Name']}  grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']}  "
                         f"block {r['Workgroup_Size_X']}x{r['Workgroup_Size_Y']}x{r['Workgroup_Size_Z']}\n")
    print(f"{len(rows)} dispatches -> {dst}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "list":
        listing(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
