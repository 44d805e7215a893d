"""Time of one PPO update of the LMPC policy (8 epochs, mini-batches of 64): the device update (csrc/lmpc_ppo.hip)
through the device-pointer entry (_lib.ppo_update_dev, data resident) and through the host entry (_lib.ppo_update,
staging included) against dart_mpc.ppo.ppo_update in torch, with the net on the GPU and on the CPU.  Same batch,
same permutations, same initial weights and Adam state for every contender and every round.
Shapes: n = 2048 (the reference's rollout_len: 256 steps) and n = 2304 (tools/lmpc_train.py 5 72 256 64).
Protocol of tools/rollout_rate.py: the contenders alternate in one process, one warm-up each, then five rounds
each; medians with the min-to-max spread.  The collection times of profiles/rollout_rate.json (the COLLECT rows)
are copied next to them: the update's share of a training iteration, before and after.
Usage: python tools/ppo_update_rate.py [out.json] [rounds]
       python tools/ppo_update_rate.py --once N     (one device update of n = N and nothing else: for a kernel trace)
       python tools/ppo_update_rate.py --collect out.json   (no GPU: copy the COLLECT rows into an existing out.json)
"""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402
from dart_mpc import _lib, ppo  # noqa: E402

HYPER = dict(clip_eps=0.2, vf_coef=0.25, ent_coef=0.01)
EPOCHS, MB = 8, 64


def make_batch(n):
    torch.manual_seed(0)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(n, 520, generator=g); obs[:, 468:] = 0.0
    with torch.no_grad():
        mean, std, _ = net(obs)
        act = mean + std * torch.randn(n, 34, generator=g)
        logp = Normal(mean, std).log_prob(act).sum(-1) + 0.15 * torch.randn(n, generator=g)
    batch = dict(obs=obs.numpy(), action=act.numpy(), logp=logp.numpy(),
                 adv=2.0 * torch.randn(n, generator=g, dtype=torch.float64).numpy(),
                 ret=5.0 + 3.0 * torch.randn(n, generator=g, dtype=torch.float64).numpy())
    return net, batch


class Contenders:
    def __init__(self, n):
        self.n = n
        self.net0, self.batch = make_batch(n)
        self.actor0, self.critic0 = ppo.pack_weights(self.net0)
        self.perms = ppo.make_perms(n, EPOCHS, torch.Generator().manual_seed(7))
        self.sample = np.arange(n, dtype=np.int32)
        self.cfg = _lib.ppo_config(epochs=EPOCHS, mini_batch_size=MB, **HYPER)
        b = self.batch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d = dict(sample=dev(self.sample), perm=dev(self.perms), obs=dev(b["obs"]), act=dev(b["action"]),
                      logp=dev(b["logp"]), adv=dev(b["adv"]), ret=dev(b["ret"]))
        self.w, self.c = dev(self.actor0), dev(self.critic0)
        self.adam = torch.zeros(2, _lib.PPO_NPARAMS, dtype=torch.float32, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stats = torch.zeros(3, dtype=torch.float64, device="cuda")
        self.ws = torch.zeros(_lib.ppo_workspace_bytes(n, MB), dtype=torch.uint8, device="cuda")
        self.w0, self.c0 = self.w.clone(), self.c.clone()
        self.losses = {}

    def device_dev(self):
        self.w.copy_(self.w0); self.c.copy_(self.c0); self.adam.zero_(); self.step.zero_()
        torch.cuda.synchronize()
        d = self.d
        t0 = time.perf_counter()
        _lib.ppo_update_dev(self.cfg, self.n, self.n, d["sample"].data_ptr(), d["perm"].data_ptr(), d["obs"].data_ptr(),
                            d["act"].data_ptr(), d["logp"].data_ptr(), d["adv"].data_ptr(), d["ret"].data_ptr(),
                            self.w.data_ptr(), self.c.data_ptr(), self.adam.data_ptr(), self.step.data_ptr(),
                            self.stats.data_ptr(), self.ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.losses["device_dev"] = self.stats.cpu().tolist()
        return dt

    def device_host(self):
        b = self.batch
        actor, critic = self.actor0.copy(), self.critic0.copy()
        adam, step = np.zeros((2, _lib.PPO_NPARAMS), np.float32), np.zeros(1, np.int32)
        t0 = time.perf_counter()
        out = _lib.ppo_update(self.cfg, self.sample, self.perms, b["obs"], b["action"], b["logp"], b["adv"], b["ret"],
                              actor, critic, adam, step)
        dt = time.perf_counter() - t0
        self.losses["device_host"] = [out["policy_loss"], out["value_loss"], out["entropy"]]
        return dt

    def _torch(self, device, name):
        net = copy.deepcopy(self.net0).to(device)
        opt = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)
        gen = torch.Generator().manual_seed(7)
        if device == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ppo.ppo_update(net, opt, self.batch, epochs=EPOCHS, mini_batch_size=MB, generator=gen, **HYPER)
        if device == "cuda":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.losses[name] = [out["policy_loss"], out["value_loss"], out["entropy"]]
        return dt

    def torch_gpu(self):
        return self._torch("cuda", "torch_gpu")

    def torch_cpu(self):
        return self._torch("cpu", "torch_cpu")


def summary(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "rounds": len(ts)}


def collect_rows():
    rows = []
    try:
        for r in json.load(open(os.path.join(ROOT, "profiles", "rollout_rate.json")))["results"]:
            if r.get("controller") == "COLLECT":
                rows.append({"B": r["B"], "steps": r["steps"], "records": r["records"],
                             "collect_wall_s": r["collect"]["wall_s"]})
    except (OSError, KeyError, ValueError):
        pass
    return rows


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--collect":
        doc = json.load(open(sys.argv[2]))
        doc["collect_of_profiles_rollout_rate_json"] = collect_rows()
        with open(sys.argv[2], "w") as f:
            json.dump(doc, f, indent=1)
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        c = Contenders(int(sys.argv[2]))
        print(f"one device update of n = {c.n}: {c.device_dev():.4f} s")
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "collect", "ppo_update_rate.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    names = ("device_dev", "device_host", "torch_gpu", "torch_cpu")
    rows = []
    for n in (2048, 2304):
        c = Contenders(n)
        for nm in names:                                    # warm-up: code objects, allocator, torch's kernels
            getattr(c, nm)()
        ts = {nm: [] for nm in names}
        for _ in range(rounds):
            for nm in names:
                ts[nm].append(getattr(c, nm)())
        row = {"n": n, "epochs": EPOCHS, "mini_batch_size": MB, "steps": EPOCHS * (-(-n // MB))}
        row.update({nm: summary(ts[nm]) for nm in names})
        row["mean_losses"] = c.losses
        med = {nm: row[nm]["median_s"] for nm in names}
        row["speedup_device_dev_over_torch_gpu"] = med["torch_gpu"] / med["device_dev"]
        row["speedup_device_dev_over_torch_cpu"] = med["torch_cpu"] / med["device_dev"]
        row["speedup_device_host_over_torch_gpu"] = med["torch_gpu"] / med["device_host"]
        row["speedup_device_host_over_torch_cpu"] = med["torch_cpu"] / med["device_host"]
        row["device_dev_us_per_step"] = 1e6 * med["device_dev"] / row["steps"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    collect = collect_rows()
    doc = {"tool": "tools/ppo_update_rate.py", "device": torch.cuda.get_device_name(0), "results": rows,
           "collect_of_profiles_rollout_rate_json": collect}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
