"""PPO on the LMPC parameter policy with the experience collected on the device: a usage example and a smoke
record, not a test.  Per iteration: collect K closed-loop steps for B controllers (LmpcSolver.collect: policy step,
solve, plant step, critic, reward, records and resets without the host), GAE on the device (_lib.gae), the
clipped-surrogate update, then the new weights go into the next collect.  --update torch (the default, so that the
recorded output stays comparable) runs dart_mpc.ppo.ppo_update and re-packs the weights; --update device runs
dart_mpc.ppo.ppo_update_device (the HIP kernels of csrc/lmpc_ppo.hip) on the packed weights in place, with the
bootstrap value from _lib.critic_value: the records, the GAE outputs and the weights never pass through torch.
--update resident runs the iterations through dart_mpc.ppo.train_device (LmpcSolver.train, csrc/lmpc_train.hip): one
call enqueues all of them -- the noise and the permutations come from the device generator, and the mean-based
parameter write and the best-policy snapshot of the reference loop are part of every iteration -- and prints the
same line per iteration from the log rows; with it --checkpoint PATH writes the training state (ppo.save_checkpoint,
one .npz without pickle) at the end and --resume PATH continues from one (the loop state and the plants start
afresh).  With --global-update (resident only) every iteration also runs the reference's second update on the
global buffer (rlmpc2.py:823-874; ppo.new_global_buffer): a quarter of its records is appended to a buffer that
survives across iterations and is updated on once it holds a full iteration's worth; the buffer is saved and resumed
with the checkpoint, so a run can stop in the middle of a fill period.
With --population P (resident only) P independent learners -- their own instances, reset pools, initial nets and
seeds (--seeds a,b,...; default 0 .. P-1) -- train in the launches of one (dart_mpc.ppo.train_population,
LmpcSolver.train_pop); a line per learner and iteration, and --checkpoint PATH writes one checkpoint per member
(PATH.member<l>.npz, each of which --resume continues alone).  --population with --global-update runs the
global-buffer update of every learner in the same launches (ppo.new_population_global_buffer); every member's
checkpoint then holds that member's buffer, so --resume --global-update continues it as a single run, in the middle
of a fill period too.
With --hyper FIELD=v[,v...] (with --population; repeatable) the learners differ in hyper-parameters: FIELD is a column
of the population's table (_lib.HYPER_FIELDS: clip_eps, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, adam_eps,
weight_decay) and takes one value for all learners or P values, one per learner -- a fixed sweep in the launches of
one run (ppo.train_population(..., hyper_table=...)).  With --pbt GENERATIONS the population is trained by
population-based training (ppo.train_pbt): per generation `iterations` training iterations, an evaluation of every
learner on held-out experiments (K steps, mean steady-state error) and the exploit/explore step, all on the device;
--pbt-replace k sets how many learners restart from the best per generation (default P / 4).  Every member's
checkpoint then holds its row of the table.
The loop state, the collection state, the targets and the plants carry over from iteration to iteration.
Prints the mean return of the episodes that ended, per iteration.
Usage: python tools/lmpc_train.py [iterations] [B] [K] [max_episode_steps] [--update device|torch|resident]
                                  [--global-update] [--checkpoint PATH] [--resume PATH] [--seed S]
                                  [--population P [--seeds a,b,...] [--hyper FIELD=v[,v...]]...
                                   [--pbt GENERATIONS [--pbt-replace k]]]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
import torch  # noqa: E402
from dart_mpc import _lib, harness, ppo  # noqa: E402
from dart_mpc.lmpc import LmpcPolicy  # noqa: E402
from dart_mpc.workload import lmpc_batch  # noqa: E402

argv = list(sys.argv[1:])
update = "torch"
if "--update" in argv:
    i = argv.index("--update")
    update = argv[i + 1]
    del argv[i:i + 2]
if update not in ("device", "torch", "resident"):
    sys.exit("--update takes device, torch or resident")


def _option(name):
    if name not in argv:
        return None
    i = argv.index(name)
    v = argv[i + 1]
    del argv[i:i + 2]
    return v


global_update = "--global-update" in argv
if global_update:
    argv.remove("--global-update")
    if update != "resident":
        sys.exit("--global-update goes with --update resident")
ckpt_out, ckpt_in, seed = _option("--checkpoint"), _option("--resume"), int(_option("--seed") or 0)
population, pop_seeds = int(_option("--population") or 0), _option("--seeds")
if population and (update != "resident" or ckpt_in):
    sys.exit("--population goes with --update resident, without --resume")
if (ckpt_out or ckpt_in) and update != "resident":
    sys.exit("--checkpoint and --resume go with --update resident")
hyper_over = {}
while "--hyper" in argv:
    spec = _option("--hyper")
    name, _, values = spec.partition("=")
    if name not in _lib.HYPER_FIELDS or not values:
        sys.exit(f"--hyper takes FIELD=v[,v...] with FIELD one of {', '.join(_lib.HYPER_FIELDS)}")
    try:
        vals = [float(v) for v in values.split(",")]
    except ValueError:
        sys.exit(f"--hyper {spec}: the values must be numbers")
    if len(vals) not in (1, population):
        sys.exit(f"--hyper {name} takes one value or {population} (one per learner), got {len(vals)}")
    hyper_over[name] = vals[0] if len(vals) == 1 else vals
pbt_generations, pbt_replace = int(_option("--pbt") or 0), _option("--pbt-replace")
if (hyper_over or pbt_generations or pbt_replace is not None) and not population:
    sys.exit("--hyper, --pbt and --pbt-replace go with --population")
if pbt_replace is not None and not pbt_generations:
    sys.exit("--pbt-replace goes with --pbt")
if pbt_generations < 0 or (pbt_replace is not None and not 0 <= 2 * int(pbt_replace) <= population):
    sys.exit("--pbt takes a positive number of generations, --pbt-replace k with 2 k <= P")
if pbt_generations and global_update:
    sys.exit("--pbt runs without --global-update")
iters = int(argv[0]) if len(argv) > 0 else 5
B = int(argv[1]) if len(argv) > 1 else 72
K = int(argv[2]) if len(argv) > 2 else 256
ep_steps = int(argv[3]) if len(argv) > 3 else 64
GAMMA, LAM, N = 0.99, 0.95, 30



def train_population():
    """P learners in one call of the population entry; member l is the single run of this script on its own data."""
    if K % int(rcfg.record_every):
        sys.exit(f"--population needs K to be a multiple of record_every = {int(rcfg.record_every)}")
    P_ = population
    sd = [int(v) for v in pop_seeds.split(",")] if pop_seeds else list(range(P_))
    if len(sd) != P_:
        sys.exit(f"--seeds needs {P_} values")
    solver = _lib.LmpcSolver(N=N, B_max=P_ * B)
    try:
        members, policies = [], []
        ns = -(-B // 18)
        for l in range(P_):
            D = lmpc_batch(ns, seed0=1000 * l)
            Q = [lmpc_batch(ns, seed0=100 + r + 1000 * l) for r in range(4)]
            torch.manual_seed(l)
            actor, critic = ppo.pack_weights(ppo.PolicyNet())
            pol = LmpcPolicy(B, weights=actor, critic_weights=critic, seed=l)
            policies.append(pol)
            members.append(dict(target=D["target"][:B], plant_pvec=D["pvec"][:B],
                                state=solver.loop_state(D["state"][:B], policy=pol),
                                cstate=solver.collect_state(np.zeros((B, 2))),
                                adam=np.zeros((2, _lib.PPO_NPARAMS), np.float32), adam_step=np.zeros(1, np.int32),
                                best=ppo.new_best(),
                                pool={"reset_x": np.stack([q["state"][:B] for q in Q]),
                                      "reset_target": np.stack([q["target"][:B] for q in Q]),
                                      "reset_pvec": np.stack([q["pvec"][:B] for q in Q])}))
        H = ppo.population_stack(members)
        gbuf = ppo.new_population_global_buffer(P_, B * (K // int(rcfg.record_every))) if global_update else None
        if gbuf is not None:
            H["global_buffer"] = gbuf
        table = _lib.hyper_table(P_, **hyper_over) if hyper_over or pbt_generations else None
        total = iters
        if pbt_generations:
            E = lmpc_batch(ns, seed0=777)               # held-out experiments, the same for every learner
            res = ppo.train_pbt(solver, policies, H, table, E["state"][:B], E["target"][:B], E["pvec"][:B], K,
                                pbt_generations, iters, sd, fitness_slot=0, steps=K, rcfg=rcfg, gamma=GAMMA, lam=LAM,
                                epochs=8, mini_batch_size=64,
                                pbt=dict(seed=seed, n_replace=int(pbt_replace or 0)))
            rows, total = res["rows"], iters * pbt_generations
        else:
            extra = dict(clip_eps=0.2, vf_coef=0.25, ent_coef=0.01) if table is None else dict(hyper_table=table)
            rows = ppo.train_population(solver, policies, H["target"], H["plant_pvec"], H["state"], H["cstate"],
                                        H["adam"], H["adam_step"], H["best"], K, sd, iterations=iters, rcfg=rcfg,
                                        pool=H["pool"], gamma=GAMMA, lam=LAM, epochs=8, mini_batch_size=64,
                                        global_buffer=gbuf, **extra)
        for j in range(total):
            for l in range(P_):
                r = rows[l][j]
                print(f"iter {j} learner {l} (seed {sd[l]}): samples {int(r['n'])}, episodes ended "
                      f"{int(r['episodes_ended'])}, mean last return {r['mean_return']:.2f}, mean step reward "
                      f"{r['mean_step_reward']:.3f}, policy loss {r['policy_loss']:.4f}, value loss "
                      f"{r['value_loss']:.4f}, entropy {r['entropy']:.3f}, best return {r['best_return']:.2f}"
                      f"{' (snapshot)' if r['snapshot'] else ''}", flush=True)
                if gbuf is not None:
                    tail = (f", update on {int(r['global_rows'])} rows: policy loss {r['global_policy_loss']:.4f}, "
                            f"value loss {r['global_value_loss']:.4f}, entropy {r['global_entropy']:.3f}"
                            if r["global_update"] else "")
                    print(f"        learner {l} global buffer {int(r['global_fill'])} rows{tail}", flush=True)
            if pbt_generations and (j + 1) % iters == 0:
                g = j // iters
                print(f"generation {g}: steady-state error {np.array2string(res['scores'][g][:, 0], precision=8)}, "
                      f"rank {res['rank'][g].tolist()}, parent {res['parent'][g].tolist()}", flush=True)
                for l in range(P_):
                    print(f"        learner {l}: " + ", ".join(f"{n} {v:.3g}" for n, v in
                                                                  zip(_lib.HYPER_FIELDS, res["hyper"][g][l])), flush=True)
        if ckpt_out:
            for l in range(P_):
                m = ppo.population_member(l, P_, H)
                st = m["state"]
                path = ppo.save_checkpoint(f"{ckpt_out}.member{l}", policies[l].weights, policies[l].critic_weights,
                                           m["adam"], m["adam_step"], m["best"], iters, st["obs_mean"], st["obs_M2"],
                                           st["obs_count"], st["history"], policies[l].current_k, st["model_params"],
                                           global_buffer=m.get("global_buffer"),
                                           hyper=None if table is None else table[l])
                print(f"checkpoint: {path} (learner {l}, best return {float(m['best']['best_return'][0]):.2f})",
                      flush=True)
    finally:
        solver.close()


rcfg = _lib.reward_config(max_episode_steps=ep_steps)
if population:
    train_population()
    sys.exit(0)

seeds = -(-B // 18)
D = lmpc_batch(seeds)
target, pvec = np.ascontiguousarray(D["target"][:B]), np.ascontiguousarray(D["pvec"][:B])
P = [lmpc_batch(seeds, seed0=100 + r) for r in range(4)]
pool = {"reset_x": np.ascontiguousarray(np.stack([p["state"][:B] for p in P])),
        "reset_target": np.ascontiguousarray(np.stack([p["target"][:B] for p in P])),
        "reset_pvec": np.ascontiguousarray(np.stack([p["pvec"][:B] for p in P]))}
rec_rows = K // int(rcfg.record_every) + 1

torch.manual_seed(0)
net = ppo.PolicyNet()
opt = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)         # rlmpc2.py:561
gen = torch.Generator().manual_seed(0)
actor, critic = ppo.pack_weights(net)
adam, adam_step = ppo.pack_adam(net, opt)                                   # (device update: a fresh Adam, zeros)
policy = LmpcPolicy(B, weights=actor, critic_weights=critic)
solver = _lib.LmpcSolver(N=N, B_max=B)
state = solver.loop_state(D["state"][:B], policy=policy)
cs = solver.collect_state(np.zeros((B, 2)))


def resident():
    """All iterations in one call of the training entry; the line per iteration comes from its log rows."""
    if K % int(rcfg.record_every):
        sys.exit(f"--update resident needs K to be a multiple of record_every = {int(rcfg.record_every)}")
    best, it0 = ppo.new_best(), 0
    gbuf = ppo.new_global_buffer(B * (K // int(rcfg.record_every))) if global_update else None
    if ckpt_in:
        c = ppo.load_checkpoint(ckpt_in)
        if c["obs_count"].shape[0] != B:
            sys.exit(f"{ckpt_in} holds {c['obs_count'].shape[0]} controllers, this run has {B}")
        policy.weights[:], policy.critic_weights[:] = c["actor"], c["critic"]
        adam[:], adam_step[:] = c["adam"], c["adam_step"]
        best = {k: c[k].copy() for k in best}
        it0 = int(c["iteration"][0])
        policy.current_k[:] = c["current_k"]
        for k in ("obs_mean", "obs_M2", "obs_count", "history", "model_params"):
            state[k][:] = c[k]
        held = ppo.global_buffer_from_checkpoint(c)
        if global_update and held is not None:
            if held["logp"].shape != gbuf["logp"].shape:
                sys.exit(f"{ckpt_in} holds a global buffer of {held['logp'].shape[0]} rows, this run needs "
                         f"{gbuf['logp'].shape[0]}")
            gbuf = held
    rows = ppo.train_device(solver, policy, target, pvec, state, cs, adam, adam_step, best, K, iterations=iters,
                            it0=it0, seed=seed, rcfg=rcfg, pool=pool, gamma=GAMMA, lam=LAM, epochs=8,
                            mini_batch_size=64, clip_eps=0.2, vf_coef=0.25, ent_coef=0.01, global_buffer=gbuf)
    for j, r in enumerate(rows):
        print(f"iter {it0 + j}: samples {int(r['n'])}, episodes ended {int(r['episodes_ended'])}, "
              f"mean last return {r['mean_return']:.2f}, mean step reward {r['mean_step_reward']:.3f}, "
              f"status != 0: {r['status_nonzero']:.4f}, policy loss {r['policy_loss']:.4f}, "
              f"value loss {r['value_loss']:.4f}, entropy {r['entropy']:.3f}, best return {r['best_return']:.2f}"
              f"{' (snapshot)' if r['snapshot'] else ''}", flush=True)
        if gbuf is not None:
            tail = (f", update on {int(r['global_rows'])} rows: policy loss {r['global_policy_loss']:.4f}, value loss "
                    f"{r['global_value_loss']:.4f}, entropy {r['global_entropy']:.3f}" if r["global_update"] else "")
            print(f"        global buffer {int(r['global_fill'])} rows{tail}", flush=True)
    if ckpt_out:
        path = ppo.save_checkpoint(ckpt_out, policy.weights, policy.critic_weights, adam, adam_step, best, it0 + iters,
                                   state["obs_mean"], state["obs_M2"], state["obs_count"], state["history"],
                                   policy.current_k, state["model_params"], global_buffer=gbuf)
        print(f"checkpoint: {path} (iteration {it0 + iters}, best return {float(best['best_return'][0]):.2f} "
              f"at iteration {int(best['best_iter'][0])})", flush=True)


try:
    if update == "resident":
        resident()
        iters = 0
    for it in range(iters):
        if update == "torch":
            policy.weights, policy.critic_weights = ppo.pack_weights(net)
        lg, clg = _lib.loop_logs(_lib.LMPC_LOOP_LOGS, K, B), _lib.loop_logs(_lib.LMPC_COLLECT_LOGS, K, B)
        rec = _lib.loop_logs(_lib.LMPC_COLLECT_REC, rec_rows, B)
        cs["nrec"][:] = 0
        noise = harness.lmpc_noise(1000 + it, K, B)
        ep0 = cs["episodes"].copy()
        solver.collect(0, K, target, pvec, state, cs, lg, clg, rec, policy, rcfg=rcfg, noise=noise, pool=pool)
        # bootstrap from the critic on the last observation (:776-779)
        last_value = (_lib.critic_value(policy.critic_weights, state["history"]) if update == "device"
                      else harness.lmpc_critic_value(policy.critic_weights, state["history"]))
        adv, ret = _lib.gae(cs["nrec"], rec["rec_reward"], rec["rec_value"], rec["rec_done"], last_value, GAMMA, LAM)
        m = np.arange(rec_rows)[:, None] < cs["nrec"][None]
        if update == "device":
            sample = np.flatnonzero(m.reshape(-1)).astype(np.int32)          # row-major: the order rec[m] gives
            out = ppo.ppo_update_device(policy.weights, policy.critic_weights, adam, adam_step, rec, sample, adv, ret,
                                        ppo.make_perms(sample.size, 8, gen), clip_eps=0.2, mini_batch_size=64,
                                        vf_coef=0.25, ent_coef=0.01)
        else:
            batch = dict(obs=rec["rec_obs"][m], action=rec["rec_action"][m], logp=rec["rec_logp"][m], adv=adv[m],
                         ret=ret[m])
            out = ppo.ppo_update(net, opt, batch, clip_eps=0.2, epochs=8, mini_batch_size=64, vf_coef=0.25,
                                 ent_coef=0.01, generator=gen)
        ended = cs["episodes"] > ep0
        mean_ret = float(cs["last_return"][ended].mean()) if ended.any() else float("nan")
        print(f"iter {it}: samples {int(m.sum())}, episodes ended {int((cs['episodes'] - ep0).sum())}, "
              f"mean last return {mean_ret:.2f}, mean step reward {float(clg['reward'].mean()):.3f}, "
              f"status != 0: {float(np.mean(lg['status'] != 0)):.4f}, policy loss {out['policy_loss']:.4f}, "
              f"value loss {out['value_loss']:.4f}, entropy {out['entropy']:.3f}", flush=True)
finally:
    solver.close()
