"""Random pushes for push-recovery training and robustness evaluation, written into a batch's body-wrench input
(SMPLSimVecEnv.enable_body_wrenches, MuJoCo's xfrc_applied).

    pushes = RandomPushes(env, bodies=["Pelvis", "Torso"], force=(50.0, 300.0), interval=(60, 120), duration=6, seed=0)
    while training:
        pushes.before_step()
        env.step(actions)

Per env a new push starts every U{a..b} control steps (start to start, drawn anew after each; the first one that many steps after
construction) — a body drawn from `bodies`, a direction uniform on the sphere, a magnitude uniform in [lo, hi] newtons, applied at
the body's centre of mass —, is held for `duration` <= a control steps and zeroed until the next one starts.  Everything is torch ops on the tensor's device, with a generator of its own
and no host synchronisation, so it can sit in a rollout loop.  Pure torch: `env` may be any object with an `xfrc_applied`
[N, nbody, 6] tensor (or an `enable_body_wrenches()` that returns one) — the schedule is tested on CPU tensors.
"""
import torch


class RandomPushes:
    def __init__(self, env, bodies, force=(50.0, 300.0), interval=(60, 120), duration=6, seed=0):
        """bodies: body indices, or names looked up in env.model.mc.body_names; force = (lo, hi) in newtons; interval = (a, b):
        control steps from the start of one push to the start of the next, drawn uniformly from {a..b}; duration <= a: control
        steps a push is held."""
        x = getattr(env, "xfrc_applied", None)
        self.xfrc = x if x is not None else env.enable_body_wrenches()
        N, nbody, six = self.xfrc.shape
        assert six == 6
        dev = self.xfrc.device
        if any(isinstance(b, str) for b in bodies):
            names = list(env.model.mc.body_names)
            bodies = [names.index(b) if isinstance(b, str) else int(b) for b in bodies]
        self.bodies = torch.as_tensor(list(bodies), dtype=torch.long, device=dev)
        if self.bodies.numel() < 1 or int(self.bodies.min()) < 0 or int(self.bodies.max()) >= nbody:
            raise ValueError("bodies must name at least one body of the model")
        self.lo, self.hi = float(force[0]), float(force[1])
        self.a, self.b, self.k = int(interval[0]), int(interval[1]), int(duration)
        if not (0 <= self.lo <= self.hi and 1 <= self.k <= self.a <= self.b):
            raise ValueError("need 0 <= lo <= hi and 1 <= duration <= a <= b")
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(int(seed))
        self._rows = torch.arange(N, device=dev)
        self.wait = self._gap(N)                              # steps left before the next push starts
        self.hold = torch.zeros(N, dtype=torch.long, device=dev)   # steps the running push is still held
        self.body = torch.zeros(N, dtype=torch.long, device=dev)
        self.push = torch.zeros(N, 3, device=dev)

    def _gap(self, n):
        return torch.randint(self.a, self.b + 1, (n,), generator=self.gen, device=self.xfrc.device)

    def before_step(self):
        """Call once before every env.step(): writes this step's pushes into env.xfrc_applied (force columns of the pushed body;
        every other entry is zero).  Returns the [N] bool mask of the envs that are pushed in this step."""
        N, dev = self.xfrc.shape[0], self.xfrc.device
        start = self.wait == 0                                # (the running push has ended: duration <= a)
        # the draws are made for every env on every call (fixed shapes, no sync) and kept where a push starts
        body = self.bodies[torch.randint(0, self.bodies.numel(), (N,), generator=self.gen, device=dev)]
        d = torch.randn(N, 3, generator=self.gen, device=dev)
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
        mag = self.lo + (self.hi - self.lo) * torch.rand(N, generator=self.gen, device=dev)
        gap = self._gap(N)
        self.body = torch.where(start, body, self.body)
        self.push = torch.where(start[:, None], d * mag[:, None], self.push)
        self.hold = torch.where(start, torch.full_like(self.hold, self.k), self.hold)
        self.wait = torch.where(start, gap, self.wait)
        active = self.hold > 0
        self.xfrc.zero_()
        self.xfrc[self._rows, self.body, :3] = self.push * active[:, None].to(self.push.dtype)
        self.hold = self.hold - active.long()
        self.wait = self.wait - 1
        return active
