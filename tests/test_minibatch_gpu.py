"""Mini-batch PPO epochs on the device (include/smplsim_mlp.h: ss_gather_rows; learning/minibatch.py; PPOConfig.use_mini_batch): the kernel bit for bit against a
torch-indexing replay on all three of its access paths, what it must leave untouched, out-of-range entries, its refusals, and the agent — the kernel's shuffle
against torch's, a mini-batch of the whole batch against the full-batch update, reproducibility from the agent's own generator, partial exploration rows."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SRC_ROWS = 1000
SENT32, SENT16 = 0x7FC0BEEF, 0x7FD5             # NaN sentinels (fp32 / bf16 bit patterns) of everything the kernel must not write


def _lib():
    from smplsim_amd._lib import lib
    return lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sources(seed=0):
    """Bit patterns, not values: random 32-bit / 16-bit words (NaN payloads, Inf, denormals among them) plus the named specials in the first rows.
    fp32 [1000, 289] dense; bf16 [1000, 384] (an operand's layout, 289 columns used); fp32 [1000, 64]; fp32 [1000, 1]."""
    g = torch.Generator().manual_seed(seed)
    w32 = lambda *s: torch.randint(-2 ** 31, 2 ** 31, s, generator=g, dtype=torch.int64).to(torch.int32)
    w16 = lambda *s: torch.randint(-2 ** 15, 2 ** 15, s, generator=g, dtype=torch.int64).to(torch.int16)
    special32 = torch.tensor([0x7FC00001, 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001, 0x807FFFFF - (1 << 32), 0x7FA00000, 0xFFFFFFFF - (1 << 32)],
                             dtype=torch.int64).to(torch.int32)
    special16 = torch.tensor([0x7FC1, 0x7F80, 0xFF80 - (1 << 16), 0x8000 - (1 << 16), 0x0001, 0x807F - (1 << 16), 0x7FA0, 0xFFFF - (1 << 16)], dtype=torch.int64).to(torch.int16)
    a, b, c, d = w32(SRC_ROWS, 289), w16(SRC_ROWS, 384), w32(SRC_ROWS, 64), w32(SRC_ROWS, 1)
    a[:8, 0] = special32; a[5, 281:289] = special32; b[:8, 0] = special16; b[7, 281:289] = special16; c[:8, 63] = special32; d[:8, 0] = special32
    return a.cuda(), b.cuda(), c.cuda(), d.cuda()


# (name, cols, ld_src, ld_dst, element bytes, which of the two block strides)
LAYOUT = [("f32_289", 289, 289, 289, 4, 0), ("bf16_289_in_384", 289, 384, 384, 2, 1), ("f32_64", 64, 64, 64, 4, 0), ("f32_1", 1, 1, 1, 4, 0)]
MARGIN = 5                                                              # destination rows beyond the last block


def _dst_rows(rows, B, stride):
    return ((rows + B - 1) // B) * stride + MARGIN


def _destinations(rows, B, strides):
    out = []
    for name, cols, lds, ldd, eb, which in LAYOUT:
        n = _dst_rows(rows, B, strides[which])
        out.append(torch.full((n, ldd), SENT32 if eb == 4 else SENT16, dtype=torch.int64).to(torch.int32 if eb == 4 else torch.int16).cuda())
    return out


def _call(srcs, dsts, perm, rows, B, strides, src_rows=SRC_ROWS):
    from smplsim_amd._cabi import GatherTensor
    table = (GatherTensor * len(srcs))()
    for j, (s, d, (name, cols, lds, ldd, eb, which)) in enumerate(zip(srcs, dsts, LAYOUT)):
        assert s.element_size() == eb and s.stride(0) == lds and d.stride(0) == ldd and s.shape[0] >= src_rows
        table[j] = GatherTensor(s.data_ptr(), d.data_ptr(), eb, cols, lds, ldd, strides[which])
    return _lib().ss_gather_rows(table, len(srcs), C.c_void_p(perm.data_ptr()), src_rows, rows, B, _st())


def _replay(srcs, dsts0, perm, rows, B, strides, src_rows=SRC_ROWS):
    """The header's row formula by torch indexing on the integer views: dst row (i // B) * stride + i % B, columns [0, cols) = src row perm[i]; rows whose entry
    is outside [0, src_rows) keep what the destination held."""
    i = torch.arange(rows, device="cuda")
    p = perm[:rows]
    ok = (p >= 0) & (p < src_rows)
    out = []
    for s, d0, (name, cols, lds, ldd, eb, which) in zip(srcs, dsts0, LAYOUT):
        drow = (i // B) * strides[which] + i % B
        d = d0.clone()
        d[drow[ok], :cols] = s[p[ok], :cols]
        out.append(d)
    return out


def _perms(rows):
    g = torch.Generator().manual_seed(rows)
    return {"identity": torch.arange(rows), "reversed": SRC_ROWS - 1 - torch.arange(rows), "random": torch.randperm(SRC_ROWS, generator=g)[:rows],
            "repeated": torch.randint(0, 40, (rows,), generator=g)}


def _check(got, want, what):
    for g, w, lay in zip(got, want, LAYOUT):
        diff = int((g != w).sum())
        assert diff == 0, (what, lay[0], diff)


# ---------------------------------------------------------------------------------------------------------------- 5: the kernel, bit for bit
@pytest.fixture(scope="module")
def srcs():
    return _sources()


# (rows, block_rows, (block stride of the fp32 tensors, of the bf16 operand))
SHAPES = [(960, 96, (96, 128)), (1000, 1000, (1000, 1024)), (960, 1, (1, 2)), (100, 96, (96, 128))]


@pytest.mark.parametrize("rows,B,strides", SHAPES)
def test_gather_rows_is_the_row_formula_bit_for_bit(srcs, rows, B, strides):
    """One call, four tensors — fp32 289 columns (4-byte units: rows do not start 16-byte aligned), bf16 289 columns in rows of 384 (2-byte units: 578 bytes are no
    multiple of 4), fp32 64 columns (16-byte units), fp32 one column (a thread per row) — for the identity, the reversed order, a random permutation and an
    index list with repeats.  Every destination, compared as integers over its WHOLE buffer, equals the torch-indexing replay: the rows and columns the call owns
    hold the source's bits (NaN payloads, +-Inf, -0.0, denormals), the pad columns, the rows between blocks and the rows after the last block keep their NaN
    sentinel.  Then the 64-column tensor again from a view that starts one element later (4-byte units): the same bytes."""
    for name, perm in _perms(rows).items():
        perm = perm.cuda()
        dsts = _destinations(rows, B, strides)
        want = _replay(srcs, dsts, perm, rows, B, strides)
        assert _call(srcs, dsts, perm, rows, B, strides) == 0, _lib().ss_last_error()
        torch.cuda.synchronize()
        _check(dsts, want, name)
        # the same call with the third source one element off a 16-byte boundary
        flat = torch.empty(SRC_ROWS * 64 + 4, dtype=torch.int32, device="cuda")
        shifted = flat[1:1 + SRC_ROWS * 64].view(SRC_ROWS, 64)
        shifted.copy_(srcs[2])
        assert shifted.data_ptr() % 16 == 4 and srcs[2].data_ptr() % 16 == 0
        dsts2 = _destinations(rows, B, strides)
        assert _call([srcs[0], srcs[1], shifted, srcs[3]], dsts2, perm, rows, B, strides) == 0, _lib().ss_last_error()
        torch.cuda.synchronize()
        _check(dsts2, want, name + " (offset source)")
        if name == "random":
            assert int((want[1][:B, 289:] == SENT16).sum()) == min(B, rows) * (384 - 289) and (want[0][-MARGIN:] == SENT32).all()   # the replay itself leaves the pads alone


# ---------------------------------------------------------------------------------------------------------------- 6: out-of-range entries
def test_out_of_range_entries_skip_their_row_and_nothing_else(srcs):
    """-1, src_rows and 2^40 at three positions of a permutation: the call returns 0, those three destination rows keep their sentinel in every tensor, every other
    row is right.  (The kernel compares an entry with [0, src_rows) before it forms an address from it: nothing out of bounds is touched.)"""
    rows, B, strides = 960, 96, (96, 128)
    perm = _perms(rows)["random"].clone()
    where = [0, 517, 959]
    perm[where[0]], perm[where[1]], perm[where[2]] = -1, SRC_ROWS, 2 ** 40
    perm = perm.cuda()
    dsts = _destinations(rows, B, strides)
    want = _replay(srcs, dsts, perm, rows, B, strides)
    assert _call(srcs, dsts, perm, rows, B, strides) == 0, _lib().ss_last_error()
    torch.cuda.synchronize()
    _check(dsts, want, "out of range")
    for d, (name, cols, lds, ldd, eb, which) in zip(dsts, LAYOUT):
        for i in where:
            assert (d[(i // B) * strides[which] + i % B] == (SENT32 if eb == 4 else SENT16)).all(), (name, i)
    # fewer source rows than the entries name: the rows beyond src_rows are skipped, not read
    dsts = _destinations(rows, B, strides)
    want = _replay(srcs, dsts, perm, rows, B, strides, src_rows=500)
    assert _call(srcs, dsts, perm, rows, B, strides, src_rows=500) == 0
    torch.cuda.synchronize()
    _check(dsts, want, "src_rows = 500")


# ---------------------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_return_invalid_and_launch_nothing():
    from smplsim_amd._cabi import GatherTensor
    L = _lib()
    src = torch.arange(1000 * 8, dtype=torch.float32, device="cuda").view(1000, 8)
    dst = torch.full((960, 8), float("nan"), device="cuda")
    perm = torch.arange(960, device="cuda")
    both = torch.zeros(2000, 8, device="cuda")
    s, d, p = src.data_ptr(), dst.data_ptr(), perm.data_ptr()
    good = dict(src=s, dst=d, eb=4, cols=8, ld_src=8, ld_dst=8, stride=96)

    def call(count=1, perm_=p, src_rows=1000, rows=960, B=96, null_table=False, n=1, **kw):
        f = dict(good, **kw)
        table = (GatherTensor * n)(*[GatherTensor(f["src"], f["dst"], f["eb"], f["cols"], f["ld_src"], f["ld_dst"], f["stride"])] * n)
        return L.ss_gather_rows(None if null_table else table, count, perm_, src_rows, rows, B, _st())

    bad = [(dict(null_table=True), b"null argument"), (dict(perm_=None), b"null argument"), (dict(src=None), b"null argument"), (dict(dst=None), b"null argument"),
           (dict(count=0), b"1 <= count <= 8"), (dict(count=9, n=9), b"1 <= count <= 8"), (dict(eb=1), b"elem_bytes"), (dict(eb=3), b"elem_bytes"), (dict(eb=8), b"elem_bytes"),
           (dict(cols=0), b"cols >= 1"), (dict(ld_src=7), b"row strides"), (dict(ld_dst=7), b"row strides"), (dict(stride=95), b"dst_block_stride"),
           (dict(src_rows=0), b"src_rows >= 1"), (dict(rows=0), b"rows >= 1"), (dict(B=0), b"block_rows >= 1"), (dict(src=s + 2), b"aligned to elem_bytes"),
           (dict(dst=d + 1, eb=2), b"aligned to elem_bytes"), (dict(perm_=p + 4), b"8-byte aligned"), (dict(dst=s), b"must not overlap"),
           (dict(src=both.data_ptr(), dst=both.data_ptr() + 32 * 999), b"must not overlap")]
    for kw, msg in bad:
        assert call(**kw) == -1 and msg in L.ss_last_error(), (kw, L.ss_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(dst).all() and torch.equal(src, torch.arange(1000 * 8, dtype=torch.float32, device="cuda").view(1000, 8)) and not both.any()
    # and the call these were variations of is accepted; neighbouring halves of one buffer do not overlap
    assert call() == 0, L.ss_last_error()
    assert call(src=both.data_ptr(), dst=both.data_ptr() + 32 * 1000) == 0, L.ss_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dst, src[:960])


# ---------------------------------------------------------------------------------------------------------------- 8 - 11: the agent
ALL_ON = dict(mfma_update=True, deterministic_update=True, fused_loss=True, fused_optimizer=True, fused_norm=True)
BASE = dict(hidden=(256, 128, 128), min_batch_size=2048, opt_num_epochs=2)


@pytest.fixture(scope="module")
def env():
    from smplsim_amd.batch import SMPLSimVecEnv
    return SMPLSimVecEnv(256, task="HumanoidSpeed", autoreset=True, seed=3)


def _agent(env, seed=1, extra=None, **cfg):
    from smplsim_amd.agents.ppo import AgentPPO, PPOConfig
    return AgentPPO(env, PPOConfig(**dict(BASE, **cfg), extra=extra or {}), seed=seed)


def _agent_state(agent):
    out = {}
    for name, net in (("policy", agent.policy_net), ("value", agent.value_net)):
        for k, v in net.state_dict().items():
            out[f"{name}.{k}"] = v
    for name, opt in (("opt_policy", agent.optimizer_policy), ("opt_value", agent.optimizer_value)):
        for i, st in enumerate(opt.state.values()):
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"{name}.{i}.{k}"] = v
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8).cpu(), b.reshape(-1).view(torch.uint8).cpu())


def _assert_same_state(a, b, what):
    torch.cuda.synchronize()
    sa, sb = _agent_state(a), _agent_state(b)
    assert sa.keys() == sb.keys() and {"policy.norm.mean", "policy.norm.n"} <= set(sa) and (what == "initial" or any(k.endswith("exp_avg_sq") for k in sa))
    differing = [k for k in sa if not _same_bits(sa[k], sb[k])]
    assert not differing, (what, differing)


def _given_perms(E, M, seed, identity=False):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.arange(M) if identity else torch.randperm(M, generator=g) for _ in range(E)]).cuda()


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


@pytest.mark.parametrize("flags", [ALL_ON, {}], ids=["library-update", "torch-update"])
def test_kernel_shuffle_equals_torch_shuffle_end_to_end(env, flags):
    """Two agents with one seed, mini_batch_size = 600 on 2048 rows (three blocks of 600 in strides of 640 for the operand, 248 rows sit out), one shuffling by
    ss_gather_rows, the other by torch indexing: clones of one rollout, the same perms, two updates — every parameter, buffer and optimiser moment bit-identical.
    With every library flag on (the critic's once-cast operand gathered as bf16), and with none (the plain torch update on the GPU)."""
    cfg = dict(flags, use_mini_batch=True, mini_batch_size=600)
    a, b = _agent(env, **cfg), _agent(env, extra={"minibatch_gather": "torch"}, **cfg)
    _assert_same_state(a, b, "initial")
    for round_ in range(2):
        batch, perms = a.sample(), _given_perms(2, 2048, 20 + round_)
        ia, ib = a.update_params(_clone(batch), perms=perms), b.update_params(_clone(batch), perms=perms)
        assert int(ia["opt_steps"]) == int(ib["opt_steps"]) == 6
        assert a._shuffled.mode == "kernel" and b._shuffled.mode == "torch" and a._shuffled.num_blocks == 3
        assert ("critic" in [s.name for s in a._shuffled.items]) == bool(flags)
        _assert_same_state(a, b, round_)
        assert float(ia["surr_loss"]) == float(ib["surr_loss"]) and float(ia["value_loss"]) == float(ib["value_loss"])


def test_a_mini_batch_of_the_whole_batch_is_the_full_batch_update(env):
    """mini_batch_size = M with the identity as every epoch's order against use_mini_batch=False, every library flag on, two updates: bit-identical states —
    the new path on the tested one."""
    mb, full = _agent(env, use_mini_batch=True, mini_batch_size=2048, **ALL_ON), _agent(env, **ALL_ON)
    for round_ in range(2):
        batch = full.sample()
        im = mb.update_params(_clone(batch), perms=_given_perms(2, 2048, 0, identity=True))
        ifull = full.update_params(_clone(batch))
        assert int(im["opt_steps"]) == int(ifull["opt_steps"]) == 2
        _assert_same_state(mb, full, round_)
        for k in ("surr_loss", "value_loss", "clip_frac", "approx_kl", "grad_norm"):
            assert float(im[k]) == float(ifull[k]), k


def test_two_agents_with_one_seed_draw_the_same_orders(env):
    """perms=None: the orders come from each agent's own update generator (seeded from the agent's seed): the same bits after an update, 2 epochs x 4 blocks of 512."""
    a, b = _agent(env, use_mini_batch=True, mini_batch_size=512, **ALL_ON), _agent(env, use_mini_batch=True, mini_batch_size=512, **ALL_ON)
    batch = a.sample()
    ia, ib = a.update_params(_clone(batch)), b.update_params(_clone(batch))
    assert int(ia["opt_steps"]) == int(ib["opt_steps"]) == 2 * 4
    _assert_same_state(a, b, "perms=None")
    assert torch.equal(a.gen_update.get_state(), b.gen_update.get_state())


def test_partial_exploration_rows(env):
    """Some rows marked as not exploration rows: with mfma_update the mini-batches' row counts would vary — ValueError, nothing updated; on the torch path every
    iteration indexes its block and the update takes opt_num_epochs * floor(M / B) steps."""
    lib_agent, torch_agent = _agent(env, use_mini_batch=True, mini_batch_size=600, **ALL_ON), _agent(env, use_mini_batch=True, mini_batch_size=600)
    batch = torch_agent.sample()
    batch["exps"][::3, ::2] = 0.0
    before = {k: v.clone() for k, v in _agent_state(lib_agent).items()}
    with pytest.raises(ValueError, match="exploration row"):
        lib_agent.update_params(_clone(batch))
    after = _agent_state(lib_agent)
    assert before.keys() == after.keys() and all(_same_bits(before[k], after[k]) for k in before)
    info = torch_agent.update_params(_clone(batch), perms=_given_perms(2, 2048, 31))
    assert int(info["opt_steps"]) == 2 * (2048 // 600)
    assert "exps" in [s.name for s in torch_agent._shuffled.items] and all(torch.isfinite(v).all() for v in _agent_state(torch_agent).values())
