"""One decode step of a Llama-style W4A8KV4 model expressed with the `qserve_backend` ops -- the bench / smoke driver.

It issues exactly the op sequence of the reference's model code for `is_prompt=False`
(qserve/modeling/models/llama_w4a8_unpad.py:185-291, 330-361, 69-93):

    rms_norm_general_fuse_sum -> qkv GEMM -> single_query_attention -> invoke_quant_fuse_sum -> o_proj GEMM
    -> residual add -> rms_norm_general_fuse_sum -> gate_up GEMM -> silu_and_mul -> invoke_quant_fuse_sum
    -> down GEMM -> residual add;   then rms_norm, fp16 lm_head, greedy sampling.

With `fuse_pairs=True` (default) the adjacent pairs (attention, quant of its output), (residual add, layer norm) and
(gate_up GEMM, silu_and_mul) are issued as one launch each (qserve_amd/fused.py) - same arithmetic, same intermediate fp16 roundings, bit-identical tensors
(tests/test_fused_gpu.py::test_decode_step_fused_pairs_equals_op_by_op; against the oracle's engine:
tests/test_loader.py::test_device_engine_matches_oracle_engine); `fuse_pairs=False` issues the reference's ops one by one.

Weights are synthetic (random packed nibbles / scales of the right shapes, distinct per layer so nothing is
served from cache); the KV cache is filled by the prefill writer.  Tensor parallelism: rank r owns
H/tp query heads, Hkv/tp KV heads and the matching column / row shards; the partial outputs of o_proj and
down_proj are summed with one RCCL all-reduce each.
"""
import os
from types import SimpleNamespace

import torch

import qserve_backend.activation_ops as activation_ops
import qserve_backend.fused_attention as fused_attention
import qserve_backend.fused_kernels as fused_kernels
import qserve_backend.layernorm_ops as layernorm_ops
import qserve_backend.qgemm_w4a8_per_chn as gemm_chn
import qserve_backend.qgemm_w4a8_per_group as gemm_grp

from . import beams as beamsmod
from . import constraints as constraintsmod
from . import drafting as draftingmod
from . import fused as fusedmod
from . import logprobs as logprobsmod
from . import lora as loramod
from . import moe as moemod
from . import paging as pagingmod
from . import penalties as penaltiesmod
from . import prefix as prefixmod
from . import rope as ropemod
from . import sampling as samplingmod
from . import serving as servingmod
from . import stopping as stoppingmod
from . import tp as tpmod
from ._lib import device_status as _device_status
from .backend._util import check as _check, lib as _lib, stream


def residual_add_(a, b):
    """a += b (fp16), the residual add the reference does with a torch add (llama_w4a8_unpad.py:348,360)."""
    _check(_lib.qs_residual_add(a.data_ptr(), b.data_ptr(), a.numel(), stream()), "residual_add")

def argmax_rows_(logits, out):
    """out[r] = argmax(logits[r]) (fp16 [rows, n] -> int64 [rows]); the greedy sampler of the benchmark step."""
    assert logits.dtype == torch.float16 and logits.dim() == 2 and logits.stride(1) == 1 and out.dtype == torch.int64
    if logits.size(1) < 8 or logits.stride(0) % 8 != 0:      # shapes the kernel's 16-byte rows cannot take (e.g. V = 32001)
        torch.argmax(logits, dim=1, out=out)
        return
    _check(_lib.qs_argmax_rows(logits.data_ptr(), out.data_ptr(), logits.size(0), logits.size(1), logits.stride(0), stream()),
           "argmax_rows")


def _tree_depths(par):
    """Depth of every node of the tree `par` (parents[i] < i, the root's is -1): the root has depth 0."""
    d = []
    for i, p in enumerate(par):
        d.append(0 if i == 0 else d[p] + 1)
    return d


LLAMA3_8B = dict(name="Llama-3-8B", hidden=4096, heads=32, kv_heads=8, inter=14336, layers=32, vocab=128256,
                 rope_theta=5e5, eps=1e-5)
LLAMA31_8B = dict(LLAMA3_8B, name="Llama-3.1-8B",
                  rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                    original_max_position_embeddings=8192))
QWEN15_72B = dict(name="Qwen1.5-72B", hidden=8192, heads=64, kv_heads=64, inter=24576, layers=80, vocab=152064,
                  rope_theta=1e6, eps=1e-6, qkv_bias=True)     # attention_bias: q/k/v projections carry a bias
LLAMA2_7B = dict(name="Llama-2-7B", hidden=4096, heads=32, kv_heads=32, inter=11008, layers=32, vocab=32000,
                 rope_theta=1e4, eps=1e-5)
LLAMA2_70B = dict(name="Llama-2-70B", hidden=8192, heads=64, kv_heads=8, inter=28672, layers=80, vocab=32000,
                  rope_theta=1e4, eps=1e-5)
TINY = dict(name="tiny-llama", hidden=256, heads=4, kv_heads=2, inter=512, layers=2, vocab=512, rope_theta=1e4,
            eps=1e-5)
# sparse MLPs (qserve_amd.moe): `experts` experts per layer, `experts_per_token` of them per token; `inter` is one expert's width
MIXTRAL_8X7B = dict(name="Mixtral-8x7B", hidden=4096, heads=32, kv_heads=8, inter=14336, layers=32, vocab=32000, rope_theta=1e6,
                    eps=1e-5, experts=8, experts_per_token=2)
TINY_MOE = dict(TINY, name="tiny-moe", experts=4, experts_per_token=2)


class W4A8Linear:
    """Stand-in for W4A8OF16LinearDynamicInputScale (w4a8_linear.py:12-134): same buffers, same call, same bias rule
    (`output_buffer += bias` after the op, :116-118 / :132-134).  Built either from synthetic random tensors or from
    checkpoint tensors (`from_tensors`, fed by qserve_amd.loader).  `defer_bias`: row-parallel shard under tensor
    parallelism - the caller adds the bias once, after the all-reduce."""

    def __init__(self, n, k, group_size, device, gen, bias=False):
        self.n, self.k, self.group_size = n, k, group_size
        self.defer_bias = False
        self.qweight = torch.randint(-128, 128, (n, k // 2), dtype=torch.int8, device=device, generator=gen)
        self.s1_scales = (torch.rand((n,), device=device, generator=gen) * 0.004 + 0.001).half()
        if group_size == -1:
            z = torch.randint(0, 16, (n,), device=device, generator=gen).half()
            self.s1_szeros = (z * self.s1_scales).half()
        else:
            # small level-2 scales keep q*s2 <= 255; any bytes are well-defined input for the kernel
            self.s2_scales = torch.randint(1, 9, (k // 128, n), dtype=torch.int8, device=device, generator=gen)
            zz = torch.randint(0, 16, (k // 128, n), device=device, generator=gen).to(torch.int16)
            self.s2_zeros = (-(zz * self.s2_scales.to(torch.int16))).to(torch.int8)
        self.bias = ((torch.rand((n,), device=device, generator=gen) - 0.5) * 0.1).half() if bias else None

    @classmethod
    def from_tensors(cls, d, group_size, defer_bias=False):
        """d: {"qweight", "s1_scales", "s1_szeros" | ("s2_scales", "s2_zeros"), ["bias"]} already on the device."""
        self = cls.__new__(cls)
        self.n, self.k, self.group_size = d["qweight"].shape[0], d["qweight"].shape[1] * 2, group_size
        self.qweight, self.s1_scales = d["qweight"], d["s1_scales"]
        if group_size == -1:
            self.s1_szeros = d["s1_szeros"]
        else:
            self.s2_scales, self.s2_zeros = d["s2_scales"], d["s2_zeros"]
            assert tuple(self.s2_scales.shape) == (self.k // 128, self.n)
        self.bias = d.get("bias")
        self.defer_bias = defer_bias
        return self

    def __call__(self, x, input_scales, input_sum, out):
        if self.group_size == -1:   # forward_per_chn, w4a8_linear.py:105-118
            gemm_chn.gemm_forward_cuda(x, self.qweight, self.s1_scales, input_scales, self.s1_szeros, input_sum, out)
        else:                       # forward_per_group, :120-134
            gemm_grp.gemm_forward_cuda(x, self.qweight, self.s2_zeros, self.s2_scales, self.s1_scales, input_scales,
                                       out)
        if self.bias is not None and not self.defer_bias:
            out += self.bias

    def planes_slices(self, tokens):
        """K slices of the planes form of this projection at `tokens` rows (0: not available / has a bias: run the pair)."""
        if self.bias is not None:
            return 0
        return fusedmod.gemm_planes_plan(tokens, self.n, self.k, self.group_size != -1)

    def planes(self, x, planes):
        """The GEMM as K-slice planes (int32 [k_slices, T, n]); its epilogue runs inside the row kernel that follows
        (`add_norm_quant_planes`)."""
        if self.group_size == -1:
            fusedmod.gemm_planes(x, self.qweight, planes)
        else:
            fusedmod.gemm_planes(x, self.qweight, planes, self.s2_zeros, self.s2_scales)

    def add_norm_quant_planes(self, out, hidden, planes, input_scales, input_sum, weight, scaling, eps, out_sum):
        """hidden += this projection's output (from its planes) ; out / scaling (/ out_sum) = rms_norm_general(hidden)."""
        if self.group_size == -1:
            fusedmod.add_residual_rms_norm_general_planes(out, hidden, planes, self.s1_scales, input_scales, weight, scaling, eps,
                                                          w_szs=self.s1_szeros, a_ssums=input_sum, input_sum=out_sum)
        else:
            fusedmod.add_residual_rms_norm_general_planes(out, hidden, planes, self.s1_scales, input_scales, weight, scaling, eps,
                                                          input_sum=out_sum)

    def silu_mul(self, x, input_scales, input_sum, out_act, tmp):
        """gate_up projection + silu_and_mul as one op (qserve_amd.fused.gemm_silu_and_mul_*): out_act [T, n/2].  Only for
        a stacked gate_up weight without bias (the bias would have to be added between the two ops)."""
        assert self.bias is None
        if self.group_size == -1:
            fusedmod.gemm_silu_and_mul_per_chn(x, self.qweight, self.s1_scales, input_scales, self.s1_szeros, input_sum,
                                               out_act, tmp)
        else:
            fusedmod.gemm_silu_and_mul_per_group(x, self.qweight, self.s2_zeros, self.s2_scales, self.s1_scales,
                                                 input_scales, out_act, tmp)


class DecodeEngine:
    def __init__(self, cfg, batch, prompt_len, max_new, group_size=-1, int4_kv=True, device="cuda:0", seed=0,
                 tp_rank=0, tp_world=1, with_lm_head=True, fuse_pairs=True, weights=None, vocab_parallel=True, planes=None,
                 direct_allreduce=None, page_pool=None, prefix_cache=False, share_pages=False):
        """weights: None = synthetic random-quantised tensors of the right shapes; otherwise this rank's tensors as
        qserve_amd.loader.load_llama_w4a8 returns them (checkpoint path).  A config with `experts` and `experts_per_token`
        (MIXTRAL_8X7B, TINY_MOE) builds mixture-of-experts layers: a router `gate` fp16 [E, hid] and two `moe.MoELinear`s in place of
        gate_up / down (weights: qserve_amd.loader.load_mixtral_w4a8); every path then runs `moe.moe_mlp` in the MLP branch of the layer
        body.  Single GPU.

        `page_pool`: None - every sequence owns ceil(max_len / 64) + 1 private pages for its whole life, and nothing below applies -, or
        N: the K and V pools of every layer hold N pages (and the sink, page N) that the rows share through `pager`, a
        `paging.PagePool`: every table entry starts at the sink, every entry that writes the cache begins with ONE reserve launch -
        step() (hence capture() / run()) for 1 token, verify_tree on both walks and speculate() (hence their captures) for the tree's n
        nodes -, and the prefill entries release every row and reserve the prompt's pages before their first layer.  While set_stopping
        is on the reserve is given `finished`: a row that is refused pages ends with stopping.NO_PAGES and is frozen from that very
        round (stop_update gives k = 0 for finished != 0); generate() reports it.  While it is off, check() raises when a row starved.
        What a frozen row guarantees under a pool is the bytes of its slots < lengths - 1: its rewrite of slot lengths - 1, and a frozen
        verification's parked nodes, may land in the sink - valid memory that only ever takes validly quantised K / V, so it stays
        finite.  Single GPU; prefill_shared refuses to run (aliased prefix pages would be released twice - the pool keeps no reference
        counts).

        `prefix_cache` (needs `page_pool`, one GPU): the pool counts the holders of every page (`paging.PagePool(refcounts=True)`: every
        reserve and release of the engine goes through the counted entries) and `self.prefix`, a `prefix.PrefixCache`, remembers which
        whole pages of 64 prompt tokens sit where: admit() maps the cached pages of a prompt's beginning into the row instead of
        recomputing them, and enters what it computed; serve() keeps a preempted row's text in the cache.  Only pages that no writer
        touches again are shared ("Prefix cache"), so there is no copy-on-write.  Off: everything launches what it did.

        `share_pages` (needs `page_pool`, one GPU): the pool counts holders as under `prefix_cache`, without a `PrefixCache` - what
        fork() and admit(copy_rows=) need to let several rows share the whole pages of one text ("Forks").  With both off
        the pool is uncounted and everything launches what it did."""
        self.cfg, self.B, self.dev = cfg, batch, torch.device(device)
        # mixture of experts: (experts, experts per token), or None for a dense model - which launches exactly what it always did
        self.moe = (int(cfg["experts"]), int(cfg["experts_per_token"])) if cfg.get("experts") else None
        if self.moe is not None:
            assert tp_world == 1, \
                "DecodeEngine: a mixture-of-experts config runs on one GPU - neither expert nor tensor parallelism of the experts is built"
            assert 1 <= self.moe[1] <= min(self.moe[0], moemod.MAX_TOP_K) and self.moe[0] <= moemod.MAX_EXPERTS, \
                f"DecodeEngine: experts={self.moe[0]} (<= {moemod.MAX_EXPERTS}), experts_per_token={self.moe[1]} (1 .. min(experts, {moemod.MAX_TOP_K}))"
        # fuse_pairs: issue (residual add + layer norm) and (silu_and_mul + quant) as one launch each
        # (qserve_amd/fused.py: bit-identical to the op pairs; False = the reference's exact op-by-op sequence)
        self.fuse_pairs = fuse_pairs
        self.tp_rank, self.tp_world = tp_rank, tp_world
        self.group_size, self.int4 = group_size, int4_kv
        H, Hkv = cfg["heads"], cfg["kv_heads"]
        # KV heads: Hkv / tp per rank, or - beyond one rank per KV head - ONE head replicated over tp / Hkv neighbouring ranks
        # (the loader's rule, qserve_amd/loader.py: rank r then holds KV head r // (tp / Hkv))
        assert H % tp_world == 0 and (Hkv % tp_world == 0 or tp_world % Hkv == 0) and \
            cfg["inter"] % (tp_world * 128) == 0, \
            f"tp_world={tp_world} must divide heads={H}, divide or be a multiple of kv_heads={Hkv}, and divide inter/128={cfg['inter'] // 128}"
        self.H, self.Hkv = H // tp_world, max(1, Hkv // tp_world)
        hid, inter = cfg["hidden"], cfg["inter"] // tp_world
        self.hid, self.inter = hid, inter
        self.qkv_n = (self.H + 2 * self.Hkv) * 128
        gen = torch.Generator(device=self.dev).manual_seed(seed + 1000 * tp_rank)
        self.layers = []
        self.with_lm_head = with_lm_head
        if weights is None:
            for _ in range(cfg["layers"]):
                self.layers.append(dict(
                    ln1=(torch.rand((hid,), device=self.dev, generator=gen) + 0.5).half(),
                    ln2=(torch.rand((hid,), device=self.dev, generator=gen) + 0.5).half(),
                    qkv=W4A8Linear(self.qkv_n, hid, group_size, self.dev, gen, bias=bool(cfg.get("qkv_bias"))),
                    o=W4A8Linear(hid, self.H * 128, group_size, self.dev, gen),
                ))
                if self.moe is None:
                    self.layers[-1].update(gate_up=W4A8Linear(2 * inter, hid, group_size, self.dev, gen),
                                           down=W4A8Linear(hid, inter, group_size, self.dev, gen))
                else:
                    self.layers[-1].update(gate=(torch.randn((self.moe[0], hid), device=self.dev, generator=gen) * hid ** -0.5).half(),   # logits of order 1
                                           gate_up=moemod.MoELinear(self.moe[0], 2 * inter, hid, group_size, self.dev, gen),
                                           down=moemod.MoELinear(self.moe[0], hid, inter, group_size, self.dev, gen))
            self.norm_w = (torch.rand((hid,), device=self.dev, generator=gen) + 0.5).half()
            if with_lm_head:
                self.embed = (torch.randn((cfg["vocab"], hid), device=self.dev, generator=gen) * 0.05).half()
                self.lm_head = (torch.randn((cfg["vocab"], hid), device=self.dev, generator=gen) * 0.02).half()
        else:
            to = lambda d: {k: v.to(self.dev).contiguous() for k, v in d.items()}   # noqa: E731
            for L in weights["layers"]:
                self.layers.append(dict(
                    ln1=L["ln1"].to(self.dev), ln2=L["ln2"].to(self.dev),
                    qkv=W4A8Linear.from_tensors(to(L["qkv"]), group_size),
                    o=W4A8Linear.from_tensors(to(L["o"]), group_size, defer_bias=tp_world > 1),
                ))
                if self.moe is None:
                    self.layers[-1].update(gate_up=W4A8Linear.from_tensors(to(L["gate_up"]), group_size),
                                           down=W4A8Linear.from_tensors(to(L["down"]), group_size, defer_bias=tp_world > 1))
                else:
                    self.layers[-1].update(gate=L["gate"].to(self.dev).half().contiguous(),
                                           gate_up=moemod.MoELinear.from_tensors(to(L["gate_up"]), group_size),
                                           down=moemod.MoELinear.from_tensors(to(L["down"]), group_size))
                    assert tuple(self.layers[-1]["gate"].shape) == (self.moe[0], hid) and self.layers[-1]["down"].experts == self.moe[0] \
                        and self.layers[-1]["gate_up"].experts == self.moe[0] and self.layers[-1]["gate_up"].n == 2 * inter
                assert self.layers[-1]["qkv"].n == self.qkv_n and self.layers[-1]["down"].k == inter
            self.norm_w = weights["norm"].to(self.dev)
            if with_lm_head:
                self.embed, self.lm_head = weights["embed"].to(self.dev), weights["lm_head"].to(self.dev)
        # ---- paged KV pools (cache_engine.py:59-115) and pointer tables (model_runner.py:396-414)
        self.max_len = prompt_len + max_new
        self.mb = (self.max_len + 63) // 64 + 1            # README.md:369 page budget rule (+1 page)
        # ---- what every rotating call takes as its rotary base: cfg["rope_theta"], or - with a `rope_scaling` (llama3, linear, yarn) - the
        # key of its frequency profile (qserve_amd/rope.py), registered on this engine's device with a table over max_len rounded up to 64
        # (content-addressed: every tensor-parallel rank gets the same key on its own device)
        self.rope_base = cfg["rope_theta"]
        prof = ropemod.profile(cfg["rope_theta"], cfg.get("rope_scaling"), cfg.get("max_pos"))
        if prof is not None:
            with torch.cuda.device(self.dev):
                self.rope_base = ropemod.register(prof[0], prof[1], (self.max_len + 63) // 64 * 64)
        dhb = 64 if int4_kv else 128
        self.size_per_token = self.Hkv * dhb
        self.page_bytes = self.Hkv * 64 * dhb + 64 * self.Hkv * 4
        assert page_pool is None or (tp_world == 1 and int(page_pool) >= 1), \
            f"DecodeEngine: page_pool={page_pool} - a page pool has at least one page and runs on one GPU (its allocator is one launch " \
            "on one device; tensor parallelism under a pool is not built)"
        assert not prefix_cache or (page_pool is not None and tp_world == 1), \
            "DecodeEngine: prefix_cache=True shares pages of a page pool - give page_pool=N; it runs on one GPU (the allocator is one " \
            "launch on one device; tensor parallelism under a pool is not built)"
        assert not share_pages or (page_pool is not None and tp_world == 1), \
            "DecodeEngine: share_pages=True shares pages of a page pool - give page_pool=N; it runs on one GPU (the allocator is one " \
            "launch on one device; tensor parallelism under a pool is not built)"
        nblocks = batch * self.mb if page_pool is None else int(page_pool) + 1       # (+ 1: the sink)
        perm = torch.randperm(batch * self.mb, generator=torch.Generator().manual_seed(seed)).reshape(batch, self.mb)
        self.pools, self.tables = [], []
        for _ in range(cfg["layers"]):
            kp = torch.zeros((nblocks, self.page_bytes), dtype=torch.uint8, device=self.dev)
            vp = torch.zeros((nblocks, self.page_bytes), dtype=torch.uint8, device=self.dev)
            t = torch.zeros((batch, 2, self.mb), dtype=torch.int64)
            if page_pool is None:
                t[:, 0] = kp.data_ptr() + perm * self.page_bytes
                t[:, 1] = vp.data_ptr() + perm * self.page_bytes
            self.pools.append((kp, vp))
            self.tables.append(t.to(self.dev))
        # page_pool: the allocator over these tables and pools (every entry the sink until a reserve), and the all-ones rows that are
        # the lengths of a prompt's reserve and the mask of a release of every row
        # prefix_cache: the host's record of the cached token chains, and per row the cached pages it holds (what `row_released` is told)
        self.pager = self._all_rows = self.prefix = None
        self._row_cached = {}
        if page_pool is not None:
            self.pager = pagingmod.PagePool(self.tables, self.pools, self.page_bytes, refcounts=bool(prefix_cache or share_pages))
            self.prefix = prefixmod.PrefixCache() if prefix_cache else None
            self._all_rows = torch.ones((batch,), dtype=torch.int32, device=self.dev)
        # ---- activation buffers (ActivationBuffer, input_metadata.py:71-109)
        B = batch
        f16, i8 = torch.float16, torch.int8
        self.hidden = torch.zeros((B, hid), dtype=f16, device=self.dev)
        self.q_act = torch.empty((B, hid), dtype=i8, device=self.dev)
        self.q_attn = torch.empty((B, self.H * 128), dtype=i8, device=self.dev)
        self.q_mlp = torch.empty((B, inter), dtype=i8, device=self.dev)
        self.q_scale = torch.empty((B,), dtype=f16, device=self.dev)
        self.q_sum = torch.empty((B,), dtype=f16, device=self.dev)
        self.qkv_buf = torch.empty((B, self.qkv_n), dtype=f16, device=self.dev)
        # row-parallel partial output / its sum over the ranks.  With the library's direct all-reduce (tp.DirectAllReduce)
        # the GEMMs write straight into the communicator's input buffer and the sum appears in its output buffer
        self.ar = direct_allreduce
        if self.ar is not None:
            assert tp_world > 1 and (B * hid) % (8 * tp_world) == 0
            self.proj_out, self.proj_res = self.ar.input((B, hid)), self.ar.output((B, hid))
        else:
            self.proj_out = torch.empty((B, hid), dtype=f16, device=self.dev)
            self.proj_res = self.proj_out
        self.gate_up_buf = torch.empty((B, 2 * inter), dtype=f16, device=self.dev)
        self.mlp_act = torch.empty((B, inter), dtype=f16, device=self.dev)
        # mixture of experts: the step's normed fp16 rows (what the router reads) and the buffers of the B * k sorted rows, persistent
        self.moe_normed = self.moe_bufs = None
        if self.moe is not None:
            self.moe_normed = torch.empty((B, hid), dtype=f16, device=self.dev)
            self.moe_bufs = moemod.mlp_buffers(B, self.moe[0], self.moe[1], hid, inter, self.dev)
        self.final = torch.empty((B, hid), dtype=f16, device=self.dev)
        # K-slice planes (qserve_amd.fused.gemm_planes): the row-parallel projections named in `planes` (default: QS_PLANES or
        # "down") leave int32 partial sums per K slice and the add + norm + quant launch behind them finishes the GEMM - where
        # the pair fusions are on, on one GPU, for shapes the library has such a launch for
        if planes is None:
            planes = tuple(x for x in os.environ.get("QS_PLANES", "down").split(",") if x)
        bad = [x for x in planes if x not in ("o", "down")]
        if bad:
            raise ValueError(f"planes / QS_PLANES: {bad} - only the row-parallel projections 'o' and 'down' have a planes form")
        self.planes = {}
        if fuse_pairs and tp_world == 1 and hid <= 4096 and hid % 2048 == 0 and self.moe is None:   # (no planes form in MoE layers)
            for name in planes:
                # one buffer serves every layer: the form is taken only if EVERY layer's projection has it with the same number
                # of slices (a layer with a bias, or of another shape, would otherwise run the planes path and lose its bias)
                ks = {layer[name].planes_slices(B) for layer in self.layers}
                if len(ks) == 1 and 0 not in ks:
                    self.planes[name] = torch.empty((ks.pop(), B, hid), dtype=torch.int32, device=self.dev)
        self.lengths = torch.full((B,), prompt_len, dtype=torch.int32, device=self.dev)   # context incl. new token
        self.tokens = torch.randint(0, cfg["vocab"], (B,), device=self.dev, generator=gen)
        # Tensor parallel: the (un-quantised) lm_head is cut over the vocabulary - rank r multiplies rows [v0, v0 + V/N)
        # only and the ranks exchange one greedy candidate per sequence (value, global index) through the SAME fp16 sum
        # all-reduce as the row-parallel partials: every rank fills its own [B, 8] slot of a zeroed [N, B, 8] tensor
        # (index split into two fp16-exact integers < 2048), so the sum is an all-gather, exact.  A replicated head made
        # every rank stream the whole 1 GB matrix for the global batch: 0.52 ms of a 3.8 ms step at N = 8.
        V = cfg["vocab"]
        self.vocab_parallel = bool(with_lm_head and tp_world > 1 and vocab_parallel and V % tp_world == 0 and
                                   V // tp_world >= 8 and (V // tp_world) % 8 == 0 and V < (1 << 22) and 8 * tp_world <= hid)
        if self.vocab_parallel:
            self.v0 = tp_rank * (V // tp_world)
            self.lm_head = self.lm_head[self.v0:self.v0 + V // tp_world].contiguous()
            self.head_idx = torch.zeros((B,), dtype=torch.int64, device=self.dev)
            n = tp_world * B * 8
            self.head_cand = self.proj_out.view(-1)[:n].view(tp_world, B, 8)      # what this rank contributes
            self.head_cand_res = self.proj_res.view(-1)[:n].view(tp_world, B, 8)  # the sum over the ranks
        # capture / capture_verify / capture_speculate: the graphs, and for each the record of what it was captured with (`_captured`)
        self.graph = self.pieces = self.verify_graph = self.speculate_graph = None
        self._step_capture = self._verify_capture = self._speculate_capture = None
        # an integer upper bound of `lengths`, kept on the host: set by the prefill entries, + 1 per step() / run(), + n per device-walk
        # verify_tree (which cannot know how many nodes were accepted without reading the device).  A planner hint and the "does it fit
        # the page tables" bound only - no result depends on it.  sync_length_bound() makes it exact again, at the price of one read-back.
        self._len_bound = prompt_len
        self._tree_cache = {}            # parent tuple -> the per-tree device constants of the device-walk verify_tree
        # append.layer_table_pointers(self.tables), built on first use (a page pool has built it)
        self._layer_tables = None if self.pager is None else self.pager.layer_tables
        self.last_verify_logits = None   # verify_tree: the logits [B, n, V] of its last call
        self.sampling = None             # set_sampling: {"seed"} while the head samples; the parameters live in device tensors:
        self._samp_t = self._samp_k = self._samp_p = self._samp_ids = None      # temperature, top-k, top-p per row; arange(B)
        self.penalties = None            # set_penalties: the (repetition, frequency, presence) device tensors while the heads penalise
        self._pen_values = None          # ... and while they do not: the same tensors, created by the first set_penalties
        # enable_drafting: the text of every sequence int32 [B, max_len], where its generated part begins int32 [B], the constants of
        # step()'s history_append, and (max_ngram, min_match, pad_token)
        self.history = self.prompt_lens = self._step_record = self._draft_params = self._prompt_len = None
        self._text_starts = None         # admit: `prompt_lens` as a host list, from the first admit on (None: all rows start at _prompt_len)
        # set_stopping: True while the stop rule runs behind the heads; its persistent device tensors (created by the first call):
        # why each sequence ended int32 [B] (stopping.LIVE / STOPPED / LENGTH), the largest text length int32 [B], the stop table, and
        # the per-step k of step()
        self.stopping = None
        self.finished = self.limit_lens = self._stop_seqs = self._stop_lens = self._stop_k = None
        # set_logprobs: (top, tempered) while the log-probability launch runs behind the heads; its persistent logs (created by the first
        # call, re-created for another `top`): float32 [B, max_len], int32 [B, max_len], int32 / float32 [B, max_len, top]; where the
        # generated text begins (the prompt length of the last prefill entry)
        self._logprobs = None
        self.logprob_log = self.rank_log = self.top_ids_log = self.top_lp_log = self._text_start = None
        # set_constraint: the device tables (token_class, next) while the heads mask - the SAME tuple as long as the same automaton is
        # on, so a capture can tell whether it was made with it -, the TokenDFA they came from, the state of every sequence int32 [B],
        # the states of a verification's nodes int32 [B * MAX_TREE]
        self._fsm = self._fsm_src = self._fsm_kept = self.fsm_state = self._fsm_node_state = None
        # enable_lora: the adapter table (lora.LoraTable) and the adapter of every sequence int32 [B] (-1: the base model), filled in
        # place; set_lora: True while lora_rows runs behind the four linears of every layer; the step's workspace
        self.lora_table = self.lora_ids = self._lora_step_ws = None
        self._lora = False
        # set_beams: the group width while the step regroups (None: off), the final ranking's length penalty, and the round's persistent
        # tensors (`_beam`: a namespace; `beam_score` float32 [B]: the sum of every row's text)
        self.beams = self._beam = self.beam_score = self.beam_parent = None
        self._beam_penalty = 1.0

    def _single_gpu(self, what):
        """What every entry behind the un-cut fp16 lm_head asks for (sampling, penalties, shared prefixes, tree verification, drafting):
        under tensor parallelism the vocabulary-parallel greedy head stays the only one."""
        assert self.with_lm_head and not self.vocab_parallel and self.tp_world == 1, f"{what}: single GPU, with the lm_head"

    # ---- the page pool (qserve_amd.paging, csrc/page_pool.hip) ---------------------------------------------------------------------
    def _reserve(self, extra):
        """The head of every entry that writes the cache, under a page pool: one `paging.PagePool.reserve` launch for the `extra` slots
        the round writes behind lengths - 1, with `finished` while the stop rule is on (a refused row freezes).  No pool: nothing."""
        if self.pager is not None:
            self.pager.reserve(self.lengths, extra, finished=self.finished if self.stopping is not None else None)

    def _prompt_pages(self, prompt_len):
        """The head of a prefill entry under a page pool: every row gives its pages back and takes those of slots 0 .. prompt_len - 1
        (two launches).  The reserve is given no `finished`, so the stop rule must be off: _prefill_entry sees to it for the prefill
        entries, prefill_cache comes here directly."""
        if self.pager is not None:
            assert self.stopping is None, \
                "a prompt's pages are reserved without the stop rule (a refused row could not be told through `finished`, and its " \
                "prompt would go to the sink) - set_stopping(None) first"
            self.release_rows(None)
            self.pager.reserve(self._all_rows, prompt_len)

    def release_rows(self, rows, drop_ids=()):
        """Give back the pages of the rows `rows` (indices; None: every row) - one launch.  Under a prefix cache the rows give up their
        HOLDS, the cache is told which cached pages they held, and `drop_ids` are the cache's own holds to drop in the same launch."""
        assert self.pager is not None, "release_rows: the engine has no page pool"
        mask = self._all_rows if rows is None else self.pager.rows_mask(rows)
        rows = list(range(self.B)) if rows is None else [int(r) for r in rows]
        if self.prefix is not None:
            for r in rows:
                self.prefix.row_released(self._row_cached.pop(r, ()))
        self.pager.release(mask, drop_ids)

    def _forkable(self, what):
        self._single_gpu(what)
        assert self.pager is not None and self.pager.refs is not None, \
            f"{what}: rows share pages of a counted page pool - DecodeEngine(page_pool=N, share_pages=True) (or prefix_cache=True)"
        assert self.history is not None, f"{what}: enable_drafting first (enable_drafting(None) for an empty batch): it writes `history`"

    def _row_tensors(self):
        """Every persistent per-row tensor that a text carries with it (those that exist)."""
        return [t for t in (self.tokens, self.lengths, self.history, self.prompt_lens, self.limit_lens, self.finished, self.fsm_state,
                            self.lora_ids, self.logprob_log, self.rank_log, self.top_ids_log, self.top_lp_log, self.hidden, self.final)
                if t is not None]

    def _fork_pages(self, pairs, lengths):
        """The fork launch for `pairs` (dst, src) over the texts' `lengths` (int32 [B]), and the host's record of the cached pages the
        new rows hold: all of the source's - they are whole prompt pages, below slot lengths - 1."""
        src_rows = torch.full((self.B,), -1, dtype=torch.int32)
        for d, s in pairs:
            src_rows[d] = s
            if self.prefix is not None:
                self._row_cached[d] = self.prefix.row_held(self._row_cached.get(s, ()))
        self.pager.fork(src_rows.to(self.dev), lengths, finished=self.finished if self.stopping is not None else None)

    def fork(self, src, rows):
        """Branch the running text of row `src` into the rows `rows` (distinct, without `src`), eagerly: they are released, every
        per-row state of `src` - tokens, lengths, history, prompt_lens, limit_lens, finished, fsm_state, lora_ids, the log-probability
        logs, hidden / final - is copied into them in place (no capture is invalidated), and ONE fork launch pair
        (`paging.PagePool.fork`) maps the source's whole pages below slot lengths - 1 into them and gives each a copy of the partly
        filled page, with `finished` while the stop rule is on: a row that cannot get its page ends with NO_PAGES (check() raises
        while the rule is off).  No copy-on-write: every writer of either text writes slots >= lengths - 1, which lie in the copied
        page or behind it.  The branches share the current token and draw their next ones under their own rows' sampler keys: they
        diverge under sampling and stay identical under greedy decoding.  Needs a counted pool (share_pages=True or prefix_cache=True)
        and enable_drafting; single GPU, with the lm_head."""
        self._forkable("fork")
        self._no_beams("fork", "the round itself decides which rows continue which texts")
        B = self.B
        src, rows = int(src), [int(r) for r in rows]
        assert 0 <= src < B and rows and len(set(rows)) == len(rows) and all(0 <= r < B for r in rows) and src not in rows, \
            f"fork: row {src} into rows {rows} - distinct row indices in 0 .. {B - 1}, the source not among them"
        self.release_rows(rows)
        rows_t = torch.tensor(rows, dtype=torch.int64, device=self.dev)
        src_t = torch.full((len(rows),), src, dtype=torch.int64, device=self.dev)
        for t in self._row_tensors():
            t.index_copy_(0, rows_t, torch.index_select(t, 0, src_t))
        if self._text_starts is not None:
            for r in rows:
                self._text_starts[r] = self._text_starts[src]
        self._fork_pages([(r, src) for r in rows], self.lengths)

    def evict_prefixes(self, pages, keep=()):
        """Evict up to `pages` cached pages that no row holds, least recently used leaves first (`prefix.PrefixCache.evict`; `keep`: ids
        to spare), and drop the cache's holds of them in one launch: each goes back to the free stack.  -> the evicted ids."""
        assert self.prefix is not None, "evict_prefixes: the engine has no prefix cache - DecodeEngine(page_pool=N, prefix_cache=True)"
        ids = self.prefix.evict(int(pages), keep)
        if ids:
            self.pager.release(torch.zeros((self.B,), dtype=torch.int32, device=self.dev), ids)
        return ids

    # ---- beam search (qserve_amd.beams, csrc/beam_select.hip) ------------------------------------------------------------------------
    def _no_beams(self, what, why):
        """What the entries refuse that cannot run while set_beams is on."""
        assert self.beams is None, f"{what}: beam search is on (set_beams) - {why}; set_beams(None) first"

    def set_beams(self, width, length_penalty=1.0):
        """Make step() / capture() / run() / generate() one round of beam search over groups of `width` rows: rows g * width ..
        g * width + width - 1 are the hypotheses of one text.  Behind the unchanged head (logits, penalties, the constraint's mask; no
        arg-max) `beams.select` picks per group the `width` best (row, token) continuations by `beam_score` + log-probability,
        `beams.move_rows` moves the per-row text state (lengths, history, prompt_lens, limit_lens, finished, fsm_state, lora_ids) of the
        rows that got another parent, in place, and the existing pool entries regroup the cache: `paging.PagePool.release(moved)`, then
        `paging.PagePool.fork(src_rows, lengths + 1)` - the whole pages shared, the tail page copied.  A row with a surviving child
        keeps its best child in place, so every source of a move stays, and where every beam keeps one child nothing moves.  A
        destination that is refused its tail page ends with finished = NO_PAGES and score -inf: the hypothesis is dropped.  A finished
        row stays in its group as a frozen row and competes with its raw sum; `length_penalty` ranks only at the end (`beam_search`).
        Everything lives in persistent device tensors: the round is captured like any other step, and `beams=width` is part of what a
        capture freezes.  `beam_score` float32 [B] is cleared to 0 by this call: every row starts as a hypothesis of its own text;
        admit() under beams starts whole groups from one prompt.

        Needs: single GPU with the lm_head; a counted pool without a prefix cache (share_pages=True) - the prefix cache's host record of
        held pages cannot follow a device-side regroup -; enable_drafting; set_stopping on; B % width == 0; sampling and set_logprobs
        off.  While on, set_sampling, set_logprobs, fork, serve, the prefill entries and the tree entries (verify_tree, speculate, their
        captures) refuse.  set_beams(None) switches it off: every path launches exactly what it launches without this call."""
        if width is None:
            self.beams = None
            return
        self._forkable("set_beams")
        width = int(width)
        assert self.prefix is None, \
            "set_beams: the engine has a prefix cache, whose host record of the pages every row holds cannot follow a regroup on the " \
            "device - DecodeEngine(page_pool=N, share_pages=True) without prefix_cache"
        assert self.stopping is not None, "set_beams: set_stopping first (finished rows stay in their group as frozen rows, and nothing else ends the search)"
        assert 1 <= width <= beamsmod.MAX_WIDTH and self.B % width == 0, \
            f"set_beams: width={width} (1 .. {beamsmod.MAX_WIDTH}) must divide the batch of {self.B} rows: rows g * width .. form group g"
        assert self.sampling is None, "set_beams: sampling is on - beams are chosen by score, not drawn; set_sampling(None) first"
        assert self._logprobs is None, "set_beams: set_logprobs is on - the logs do not follow a regroup; set_logprobs(None) first"
        assert self.cfg["vocab"] >= 8 and self.cfg["vocab"] % 8 == 0, "set_beams: the logit rows need a vocabulary that is a multiple of 8"
        B, dev = self.B, self.dev
        if self._beam is None or self._beam.cand_ids.size(1) != width:
            i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
            self._beam = SimpleNamespace(
                score_out=torch.zeros((B,), **f32), parent=torch.zeros((B,), **i32), next_token=torch.zeros((B,), dtype=torch.int64, device=dev),
                moved=torch.zeros((B,), **i32), src_rows=torch.full((B,), -1, **i32), cand_ids=torch.full((B, width), -1, **i32),
                cand_lp=torch.zeros((B, width), **f32), lens=torch.zeros((B,), **i32))
        if self.beam_score is None:
            self.beam_score = torch.zeros((B,), dtype=torch.float32, device=dev)
        self.beam_score.zero_()
        self.beam_parent = self._beam.parent                                # (the last round's parents, for callers that follow the regroup)
        self.beams, self._beam_penalty = width, float(length_penalty)

    def _beam_moved_tensors(self):
        """The per-row text state that the launches behind the regroup read (those that exist); `tokens` is written from the
        selection, `hidden` / `final` are derived from it by the next step."""
        return [t for t in (self.lengths, self.history, self.prompt_lens, self.limit_lens, self.finished, self.fsm_state, self.lora_ids)
                if t is not None]

    def _beam_round(self, logits):
        """The regroup of one beam round, between the head and the tail of step(): select, move, unhold, fork, and the new tokens and
        scores - nothing read back.  Slot lengths - 1 was written by this step and belongs to the child: the fork is
        told lengths + 1, so its rule w = (len - 1) / 64, t = (len - 1) % 64 carries that slot."""
        bm = self._beam
        torch.add(self.lengths, 1, out=bm.lens)
        beamsmod.select(logits, self.beam_score, self.finished, self.tokens, self.beams,
                        out=(bm.parent, bm.next_token, bm.score_out, bm.moved, bm.src_rows, bm.cand_ids, bm.cand_lp))
        beamsmod.move_rows(bm.parent, self._beam_moved_tensors(), self.pager.error)
        self.pager.release(bm.moved)
        self.pager.fork(bm.src_rows, bm.lens, finished=self.finished)
        # a destination that was refused its tail page holds nothing (finished = NO_PAGES by the fork): its hypothesis is dropped
        bm.score_out.masked_fill_((bm.moved != 0) & (self.pager.starved != 0), float("-inf"))
        self.beam_score.copy_(bm.score_out)
        self.tokens.copy_(bm.next_token)

    def beam_search(self, max_rounds, poll_every=8):
        """generate() under set_beams, and the final ranking: per group the hypotheses that are alive (score above -inf), best first by
        `beams.rank` - score / max(generated tokens, 1) ** length_penalty in float64, ties by row.
        -> (groups: per group a list of (tokens, cum_score, final_score, reason) - the generated tokens as generate() returns them, the
        raw sum, the ranked score, `finished` -; rounds; read_backs)."""
        assert self.beams is not None, "beam_search: set_beams first"
        texts, reasons, rounds, reads = self.generate(max_rounds, poll_every=poll_every)
        cum = self.beam_score.cpu().tolist()
        W, groups = self.beams, []
        for g in range(self.B // W):
            rows = list(range(g * W, g * W + W))
            order, scores = beamsmod.rank([cum[b] for b in rows], [len(texts[b]) for b in rows], self._beam_penalty)
            groups.append([(texts[rows[i]], cum[rows[i]], scores[i], reasons[rows[i]]) for i in order if cum[rows[i]] != float("-inf")])
        return groups, rounds, reads

    # ---- the sampling head (qserve_amd.sampling, csrc/sample_rows.hip) --------------------------------------------------------
    def set_sampling(self, temperature, top_k=0, top_p=1.0, seed=0):
        """Make the head of step() / capture() / run(), of the prefill entries and of verify_tree(sampled=True) draw from the
        temperature / top-k / top-p distribution (`sampling.sample_rows`) instead of taking the arg-max; set_sampling(None) goes back to
        greedy.  The three values live in persistent device tensors that are filled in place, so a captured graph sees later changes of
        them; whether the head samples at all, and `seed`, are frozen into a capture - capture after switching, re-capture for another
        seed.  The randomness of a token is a function of (seed, sequence, position) alone (`sampling.position_keys`): a captured step
        advances it by advancing `lengths`, and the token sequence does not depend on what verify_tree was given as a draft, up to the
        numerics of the append path against the decode path - a draft only decides how many positions one pass yields.  Single GPU, with
        the lm_head; under tensor parallelism the greedy head stays the only one."""
        if temperature is None:
            self.sampling = None
            return
        self._no_beams("set_sampling", "beams are chosen by score, not drawn (sampled beams are out of scope)")
        self._single_gpu("set_sampling")
        from .append import MAX_TREE
        if self._samp_t is None:
            rows = self.B * MAX_TREE                      # (verify_tree samples B * n rows, n <= MAX_TREE)
            self._samp_t = torch.empty((rows,), dtype=torch.float32, device=self.dev)
            self._samp_k = torch.empty((rows,), dtype=torch.int32, device=self.dev)
            self._samp_p = torch.empty((rows,), dtype=torch.float32, device=self.dev)
            self._samp_ids = torch.arange(self.B, dtype=torch.int64, device=self.dev)
        self._samp_t.fill_(float(temperature))
        self._samp_k.fill_(int(top_k))
        self._samp_p.fill_(float(top_p))
        self.sampling = dict(seed=int(seed))

    def _sample(self, logits, out, keys):
        """out[r] = the token drawn from row r of `logits` under the engine's sampling parameters and the Philox key keys[r]."""
        rows = logits.size(0)
        samplingmod.sample_rows(logits, out, self._samp_t[:rows], self._samp_k[:rows], self._samp_p[:rows], seed=self.sampling["seed"],
                                row_keys=keys)

    def _step_keys(self):
        """The keys of the tokens the head is about to draw: (b, lengths[b]) - the position the new token will hold."""
        return samplingmod.position_keys(self._samp_ids, self.lengths)

    def _head(self, final, out, keys=None, draft=(), penalise=True, choose=True):
        """The head of every path but the vocabulary-parallel one: the un-quantised fp16 lm_head on the normed rows `final`
        (llama_w4a8_unpad.py:392,476), the penalty launch while set_penalties is on (`draft`: the drafted tokens and the tree of a
        verification; a step's context is the text alone; the prefill entries and the host-walk verify_tree refuse to run while penalties
        are on, so their heads never penalise; `penalise=False`: the head of an admission, which runs while they are on and draws its
        token before the new text's history is complete), then out[r] = the arg-max of row r or, with `keys`, the token drawn under the
        Philox keys keys() - computed behind the logits, from the lengths as they stand then.  While set_constraint is on the mask
        launch runs behind the penalties: every row under the automaton state of its own node - `fsm_state` for a step and for the
        prompt head, the states along the draft's paths for a verification.  `choose=False`: no token is chosen, `out` is not written.
        -> the logits (penalised and masked, while on)."""
        logits = torch.matmul(final, self.lm_head.t())
        if penalise and self.penalties is not None:
            self._penalize(logits, *draft)
        if self._fsm is not None:
            self._constrain(logits, *draft)
        if not choose:                                               # (set_beams: the round chooses over groups of rows, behind the head)
            return logits
        if keys is not None:
            self._sample(logits, out, keys())
        else:
            argmax_rows_(logits, out)                                # greedy sampler
        return logits

    # ---- fill the cache for positions [0, prompt_len) through the prefill writer (random K/V source) ----------
    def prefill_cache(self, prompt_len, chunk=8):
        B = self.B
        self._prompt_pages(prompt_len)
        gen = torch.Generator(device=self.dev).manual_seed(99)
        seq = torch.full((B,), prompt_len, dtype=torch.int32, device=self.dev)
        cu = (torch.arange(0, B + 1, device=self.dev, dtype=torch.int32) * prompt_len)
        pad = fused_attention.compute_padding_offsets(cu, prompt_len, B * prompt_len)
        qkv = torch.randn((B * prompt_len, self.qkv_n), dtype=torch.float16, device=self.dev, generator=gen)
        for li in range(self.cfg["layers"]):
            work = qkv if li == 0 else (qkv * (1.0 + 0.01 * li)).half()
            fused_attention.apply_bias_rope_update_kv_cache(
                work, seq, pad, self.tables[li], self.H, self.Hkv, prompt_len, 64, self.size_per_token, 128,
                self.rope_base, 8192, True, self.int4, True)
        self.lengths.fill_(prompt_len + 1)
        self._len_bound = prompt_len + 1
        torch.cuda.synchronize()

    # ---- real prefill: the reference's is_prompt=True path (llama_w4a8_unpad.py:199-243, 330-361) -------------
    def _prompt_buffers(self, T):
        """Activation buffers of the is_prompt path for T rows."""
        f16, i8, dev = torch.float16, torch.int8, self.dev
        bufs = dict(
            qa=torch.empty((T, self.hid), dtype=i8, device=dev), qo=torch.empty((T, self.H * 128), dtype=i8, device=dev),
            q_scale=torch.empty((T,), dtype=f16, device=dev),
            q_sum=torch.empty((T,), dtype=f16, device=dev), qkv=torch.empty((T, self.qkv_n), dtype=f16, device=dev),
            proj=torch.empty((T, self.hid), dtype=f16, device=dev))
        if self.moe is not None:                                     # the T * k sorted rows live in `moe` (moe.mlp_buffers)
            bufs.update(normed=torch.empty((T, self.hid), dtype=f16, device=dev),
                        moe=moemod.mlp_buffers(T, self.moe[0], self.moe[1], self.hid, self.inter, dev))
        else:
            bufs.update(q_mlp=torch.empty((T, self.inter), dtype=i8, device=dev),
                        gate_up=torch.empty((T, 2 * self.inter), dtype=f16, device=dev),
                        mlp_act=torch.empty((T, self.inter), dtype=f16, device=dev))
        return bufs

    def _quant(self, out, x, q_sum, q_scale):
        """out / q_scale (/ q_sum: per-channel weights only) = the per-token int8 quantisation of the fp16 rows x."""
        if self.group_size == -1:
            fused_kernels.invoke_quant_fuse_sum(out, x, q_sum, q_scale)
        else:
            fused_kernels.invoke_quant(out, x, q_scale)

    def _layer_stack(self, h, bufs, attention, planes, lora_ids=None):
        """THE transformer layer body (llama_w4a8_unpad.py:330-361 per layer), in place on the fp16 rows h - every path of the engine
        runs this one generator.  `bufs`: the activation buffers under the keys of _prompt_buffers, of exactly h's rows, plus "proj_res",
        where the sum of the row-parallel partial "proj" over the ranks is read from (the same tensor unless a collective writes
        elsewhere).  attention(li, qkv): cache write + attention of layer li on its packed qkv rows, leaving the QUANTISED output in
        bufs["qo"] / ["q_scale"] / ["q_sum"].  `planes`: name -> K-slice plane buffer of the row-parallel projections that run as
        planes (the decode step's; empty elsewhere).  Yields the partial wherever tensor parallelism needs its sum all-reduce (2 per
        layer; nothing at world size 1), so that the caller decides how the collective is issued.  `lora_ids`: as for _lora_plan."""
        eps = self.cfg["eps"]
        fuse_sum, fuse = self.group_size == -1, self.fuse_pairs
        qa, qo, q_mlp, q_scale, q_sum, qkv, proj, proj_res, gate_up, mlp_act = (
            bufs.get(k) for k in ("qa", "qo", "q_mlp", "q_scale", "q_sum", "qkv", "proj", "proj_res", "gate_up", "mlp_act"))
        sums = q_sum if fuse_sum else None
        # set_lora: lora_rows behind every base GEMM (and its bias), on that GEMM's quantised input.  A linear with an adapter takes the
        # path a linear with a bias takes: no planes form, no silu * mul epilogue - the delta has to be added in between
        lora = self._lora_plan(h.size(0), lora_ids) if self._lora else None

        def lora_add(li, name, out, xq):
            if lora is not None:
                A, B = self.lora_table.layers[li][name]
                loramod.lora_rows(out, xq, q_scale, A, B, self.lora_table.scaling, lora[0], lora[1], self.lora_table.shapes[name][2],
                                  workspace=lora[2])

        def norm_quant(x, w):
            if fuse_sum:
                layernorm_ops.rms_norm_general_fuse_sum(qa, x, w, q_sum, q_scale, eps, True)
            else:
                layernorm_ops.rms_norm_general(qa, x, w, q_scale, eps, True)

        def add_norm_quant(x, delta, w):
            if fuse:
                fusedmod.add_residual_rms_norm_general(qa, x, delta, w, q_scale, eps, sums)
            else:
                residual_add_(x, delta)
                norm_quant(x, w)

        # (row-parallel GEMM, add + norm + quant) as K-slice planes: the GEMM leaves int32 partial sums per K slice, the row
        # kernel that follows sums them and applies the GEMM's epilogue (bit-identical pair fusion; single GPU only - under
        # tensor parallelism the all-reduce sits between the two)
        def proj_add_norm_quant(lin, name, xq, x, w):
            pl = planes.get(name) if fuse and self.tp_world == 1 and lora is None else None
            if pl is not None:
                lin.planes(xq, pl)
                lin.add_norm_quant_planes(qa, x, pl, q_scale, q_sum, w, q_scale, eps, sums)
                return True
            return False

        def row_parallel(li, name, lin, xq):
            """lin(xq) -> the rows to add to h: the projection's output or, under tensor parallelism, its sum over the ranks."""
            lin(xq, q_scale, q_sum, proj)
            if self.tp_world == 1:
                lora_add(li, name, proj, xq)                         # (set_lora is single GPU)
                return proj
            yield proj
            if lin.defer_bias and lin.bias is not None:
                proj_res.add_(lin.bias)                              # once, after the reduce
            return proj_res

        nl = len(self.layers)
        for li, L in enumerate(self.layers):
            if li == 0:
                norm_quant(h, L["ln1"])
            L["qkv"](qa, q_scale, q_sum, qkv)
            lora_add(li, "qkv", qkv, qa)
            attention(li, qkv)
            if self.moe is not None:
                # the sparse MLP (mixtral_w4a8_unpad.py:279-374): the router reads the UN-quantised normed rows, the experts the quantised
                # ones; `moemod.moe_mlp` is looked up per call (the seam tests wrap)
                res = yield from row_parallel(li, "o", L["o"], qo)
                residual_add_(h, res)
                layernorm_ops.rms_norm(bufs["normed"], h, L["ln2"], eps)
                logits = torch.matmul(bufs["normed"], L["gate"].t())
                self._quant(qa, bufs["normed"], q_sum, q_scale)
                moemod.moe_mlp(proj, qa, q_scale, sums, logits, self.moe[1], L["gate_up"], L["down"], bufs["moe"])
                if li + 1 < nl:
                    add_norm_quant(h, proj, self.layers[li + 1]["ln1"])   # next layer's input norm
                else:
                    residual_add_(h, proj)
                continue
            if not proj_add_norm_quant(L["o"], "o", qo, h, L["ln2"]):
                res = yield from row_parallel(li, "o", L["o"], qo)
                add_norm_quant(h, res, L["ln2"])
            plain = L["gate_up"].bias is not None or lora is not None   # something is added between the GEMM and silu * mul
            if fuse and not plain:                     # gate_up GEMM with the silu * mul epilogue, then the quantiser
                L["gate_up"].silu_mul(qa, q_scale, q_sum, mlp_act, gate_up)
            else:
                L["gate_up"](qa, q_scale, q_sum, gate_up)
                lora_add(li, "gate_up", gate_up, qa)
            if fuse and plain:
                fusedmod.silu_and_mul_quant(q_mlp, gate_up, q_scale, sums)
            else:
                if not fuse:
                    activation_ops.silu_and_mul(mlp_act, gate_up)
                self._quant(q_mlp, mlp_act, q_sum, q_scale)
            if li + 1 < nl and proj_add_norm_quant(L["down"], "down", q_mlp, h, self.layers[li + 1]["ln1"]):
                continue                                             # (next layer's input norm done from the planes)
            res = yield from row_parallel(li, "down", L["down"], q_mlp)
            if li + 1 < nl:
                add_norm_quant(h, res, self.layers[li + 1]["ln1"])   # next layer's input norm
            else:
                residual_add_(h, res)

    def _prompt_layers(self, h, bufs, attend, lora_ids=None):
        """The layer stack of the is_prompt path, in place on h (fp16 [T, hid]); `bufs`: _prompt_buffers of >= T rows.
        attend(li, qkv) -> fp16 [T, H * 128]: cache write + attention of layer li on its packed qkv rows (prefill: writer + flash
        over the call's own k / v; prefill_chunked: append attention over the pages + the chunk).  The row-parallel partials are
        summed through the process group, in place.  `lora_ids`: as for _lora_plan."""
        b = {k: v[:h.size(0)] for k, v in bufs.items() if k != "moe"}
        b["proj_res"] = b["proj"]
        if self.moe is not None:
            b["moe"] = moemod.slice_buffers(bufs["moe"], h.size(0), self.moe[1])

        def attention(li, qkv):
            self._quant(b["qo"], attend(li, qkv), b["q_sum"], b["q_scale"])

        for partial in self._layer_stack(h, b, attention, {}, lora_ids):
            tpmod.all_reduce_sum_(partial)

    def _prefill_entry(self, what):
        """What every prefill entry refuses BEFORE it touches the cache: penalties on - the head of a prefill draws its token before
        the new prompt's history exists, so it could not penalise."""
        self._no_beams(what, "a beam's first tokens are chosen by admit() over whole groups")
        assert self.penalties is None, \
            f"{what}: the prefill head does not penalise (the history of the new prompt does not exist yet) - set_penalties(None), " \
            "prefill, enable_drafting, then set_penalties again"
        assert self.stopping is None, \
            f"{what}: the stop rule reads the history of the prompt it was switched on for - set_stopping(None), prefill, " \
            "enable_drafting, then set_stopping again"

    def _prompt_head(self, last_rows, prompt_len, rows=None):
        """The head behind a prompt pass: last-token states -> `hidden`, first sampled token -> `tokens`, lengths = prompt_len + 1.
        `rows` None: every row, a prefill entry - written in place, `prompt_len` an int.  Else (admit): the rows `rows` (int64 [R]) alone,
        `prompt_len` int32 [R]: the full-batch head runs on copies with k = 1 on those rows and 0 elsewhere, and its results are merged
        into them - every other row keeps its bytes.  Either way: the constraint's mask under `fsm_state`, sampler keys (row, prompt
        length), no penalties; the tail records the token at column prompt_len of the rows' cleared logs and advances `fsm_state` once;
        the stop rule does not run here (admit's root check follows it)."""
        if rows is None:
            hidden, final, out, pos, k = self.hidden, self.final, self.tokens, self.lengths, None
            hidden.copy_(last_rows)
            pos.fill_(prompt_len)                                    # the first new token will hold position prompt_len
        else:
            hidden, final, out, pos = self.hidden.clone(), torch.empty_like(self.final), self.tokens.clone(), self.lengths.clone()
            hidden[rows], pos[rows] = last_rows, prompt_len
            k = torch.zeros_like(pos)
            k[rows] = 1
        layernorm_ops.rms_norm(final, hidden, self.norm_w, self.cfg["eps"])
        if self.vocab_parallel:                                      # (a prefill entry: admit is single GPU)
            tpmod.all_reduce_sum_(self._head_local())                # in place, through the process group
            self._head_finish(self.head_cand)
        else:
            keys = (lambda: samplingmod.position_keys(self._samp_ids, pos)) if self.sampling is not None else None
            beam = self.beams is not None and rows is not None       # (admit under set_beams; the prefill entries refuse)
            logits = self._head(final, out, keys, penalise=False, choose=not beam)
            if beam:                                                 # a group's first tokens: the leader's W best, slot i the i-th
                cum = torch.full((self.B,), float("-inf"), dtype=torch.float32, device=self.dev)
                cum[rows[rows % self.beams == 0]] = 0.0              # the followers are copies of the leader: only it has candidates
                res = beamsmod.select(logits, cum, torch.zeros_like(pos), out, self.beams)
                out.copy_(res[1])
                self.beam_score[rows] = torch.index_select(res[2], 0, rows)
            if self._logprobs is not None:                           # a new text: the first token's entry lands at column prompt_len
                self._clear_logprob_logs(rows)
            self._emit(logits, out, lengths=pos, k=k)                # (a prefill entry: stopping is off, by _prefill_entry)
        if rows is None:
            self.lengths.fill_(prompt_len + 1)
            self._len_bound = prompt_len + 1
            self._text_start, self._text_starts = prompt_len, None
        else:
            self.hidden[rows], self.final[rows], self.tokens[rows] = last_rows, torch.index_select(final, 0, rows), torch.index_select(out, 0, rows)
            self.lengths[rows] = prompt_len + 1

    def prefill(self, prompt_len, tokens=None):
        """Run the prompt through the model: per layer  norm+quant -> qkv GEMM -> apply_bias_rope_update_kv_cache
        (RoPE in place + quantised cache write) -> flash_attn_varlen_func (causal) -> quant -> o_proj -> residual+norm
        -> gate_up -> silu_and_mul+quant -> down -> residual.  All sequences have `prompt_len` tokens.  Leaves the
        cache filled, `hidden` = last-token states, `tokens` = first sampled token, lengths = prompt_len + 1."""
        from .flash import flash_attn_varlen_func
        self._prefill_entry("prefill")
        cfg, B, dev = self.cfg, self.B, self.dev
        assert self.with_lm_head and prompt_len + 1 <= self.max_len
        T = B * prompt_len
        if tokens is None:
            tokens = torch.randint(0, cfg["vocab"], (T,), device=dev,
                                   generator=torch.Generator(device=dev).manual_seed(7))
        self._prompt_pages(prompt_len)
        h = torch.index_select(self.embed, 0, tokens)
        bufs = self._prompt_buffers(T)
        seq = torch.full((B,), prompt_len, dtype=torch.int32, device=dev)
        cu = torch.arange(0, B + 1, device=dev, dtype=torch.int32) * prompt_len
        pad = fused_attention.compute_padding_offsets(cu, prompt_len, T)

        def attend(li, qkv):
            fused_attention.apply_bias_rope_update_kv_cache(
                qkv, seq, pad, self.tables[li], self.H, self.Hkv, prompt_len, 64, self.size_per_token, 128,
                self.rope_base, 8192, True, self.int4, True)
            q, k, v = qkv.split([self.H * 128, self.Hkv * 128, self.Hkv * 128], dim=-1)
            return flash_attn_varlen_func(q.reshape(T, self.H, 128), k.reshape(T, self.Hkv, 128),
                                          v.reshape(T, self.Hkv, 128), cu, cu, prompt_len, prompt_len, dropout_p=0.0,
                                          causal=True).reshape(T, -1)

        self._prompt_layers(h, bufs, attend)
        last = (cu[1:] - 1).to(torch.int64)
        self._prompt_head(torch.index_select(h, 0, last), prompt_len)

    def prefill_chunked(self, prompt_len, chunk, tokens=None):
        """`prefill` in chunks of `chunk` tokens per sequence (the last one may be shorter): the same op sequence per chunk on
        B * chunk rows - the activations never hold more -, attention through qserve_amd.append.append with past = c * chunk
        (the chunk's K / V go into the pages, its queries attend to the pages of the earlier chunks and, in fp16, to the chunk
        itself); lm_head and sampling once, after the last chunk.  Ends in the state `prefill` ends in.  `tokens`: as for
        `prefill`, [B * prompt_len], sequence-major."""
        self._prefill_entry("prefill_chunked")
        cfg, B, dev = self.cfg, self.B, self.dev
        assert self.with_lm_head and prompt_len + 1 <= self.max_len and chunk >= 1
        if tokens is None:
            tokens = torch.randint(0, cfg["vocab"], (B * prompt_len,), device=dev,
                                   generator=torch.Generator(device=dev).manual_seed(7))
        chunk = min(chunk, prompt_len)
        self._prompt_pages(prompt_len)
        last = self._prompt_pass(tokens.view(B, prompt_len), [prompt_len] * B, chunk, self._prompt_buffers(B * chunk), 0,
                                 self._append_over(self.tables))
        self._prompt_head(last, prompt_len)

    def _append_over(self, tables, past0=0):
        """The `attend` of a _prompt_pass that is `append.append` over the pass's sequences' rows of tables[li]; `past0`: the largest
        `base` of the pass's sequences (the hint is a bound of base + c0)."""
        from . import append as appendmod      # (looked up per call: `appendmod.append` is the seam tests wrap)
        # (max_past = c0, known on the host: a long past at a small batch is cut into page ranges - append_attention_split.hip)
        def attend(li, qkv, cu, past, n, c0, live):
            return appendmod.append(qkv, cu, past, tables[li] if live is None else tables[li][live], self.H, self.Hkv, self.size_per_token,
                                    self.rope_base, self.int4, max_seqlen_q=n, max_past=past0 + c0)
        return attend

    def _prompt_pass(self, tokens, lens, chunk, bufs, base, attend, lora_ids=None):
        """THE chunked prompt pass: the layer stack over R sequences of possibly different lengths, `tokens` [R, >= max(lens)] on the
        device (padded; sequence r is tokens[r, :lens[r]]) and `lens` a host list, in passes of `chunk` columns: pass c0 runs
        tokens[r, c0 : c0 + chunk] of every sequence that has a token left - one with none is left out -, behind a past of base + c0
        (`base`: an int, or one int per sequence - what already sits in its pages),
        with cu_seqlens from the pass's lengths.  attend(li, qkv, cu_seqlens, past_lens, n, c0, live) -> fp16 [T, H, 128]: the append
        attention of layer li over the pass's T rows; n: the longest sequence of the pass; `live`: the sequences in it, int64 indices
        on the device, or None when all are.  `bufs`: _prompt_buffers of at least R * chunk rows.  `lora_ids`: the adapter of every
        SEQUENCE int32 [R], handed on per token (None: the engine's, which needs equal lengths).  -> every sequence's last hidden row,
        gathered where the sequence ends, [R, hid]."""
        R, dev = len(lens), self.dev
        last = torch.empty((R, self.hid), dtype=torch.float16, device=dev)
        for c0 in range(0, max(lens), chunk):
            live = [r for r in range(R) if lens[r] > c0]
            ns = [min(chunk, lens[r] - c0) for r in live]
            cu_h = [sum(ns[:j]) for j in range(len(ns) + 1)]
            T, n = cu_h[-1], max(ns)
            h = torch.index_select(self.embed, 0, torch.cat([tokens[r, c0:c0 + m] for r, m in zip(live, ns)]))
            cu = torch.tensor(cu_h, dtype=torch.int32, device=dev)
            past = torch.full((len(live),), base + c0, dtype=torch.int32, device=dev) if isinstance(base, int) else \
                torch.tensor([base[r] + c0 for r in live], dtype=torch.int32, device=dev)
            live_t = None if len(live) == R else torch.tensor(live, dtype=torch.int64, device=dev)
            ids = None if lora_ids is None else torch.repeat_interleave(     # the adapter of every token of this pass
                lora_ids if live_t is None else torch.index_select(lora_ids, 0, live_t), torch.tensor(ns, dtype=torch.int64, device=dev), output_size=T)
            self._prompt_layers(h, bufs, lambda li, qkv: attend(li, qkv, cu, past, n, c0, live_t).reshape(T, -1), ids)
            ended = [(r, cu_h[j + 1] - 1) for j, r in enumerate(live) if c0 + ns[j] == lens[r]]
            if ended:
                last[torch.tensor([r for r, _ in ended], dtype=torch.int64, device=dev)] = \
                    torch.index_select(h, 0, torch.tensor([e for _, e in ended], dtype=torch.int64, device=dev))
        return last

    def prefill_shared(self, prefix_tokens, suffix_tokens, chunk=None):
        """`prefill_chunked` for B prompts that begin with the SAME `prefix_tokens` [P] and go on with their own `suffix_tokens`
        [B, S] (S >= 1), the common part computed and stored once.  With P64 = 64 * (P // 64), the whole pages of the prefix:
          1. the first P64 prefix tokens run ONCE, as a single sequence over row 0 of the page tables (chunks through `append`);
          2. entries < P64 / 64 of every sequence's K and V table rows are pointed at sequence 0's pages, in every layer;
          3. every sequence's remaining P - P64 prefix tokens and its S suffix tokens run in chunks through `append_shared` with one
             group of B, prefix P64 and past = P64 + c0: the shared pages are read once per layer and chunk for the whole batch.
        Ends in the state `prefill` ends in (`hidden`, `tokens`, lengths = P + S + 1); step() / capture() / run() go on unchanged - the
        decode kernels only read the aliased pages and write at slots >= P64.  `chunk`: tokens per sequence and pass (None: no
        chunking).  Single GPU, with the lm_head."""
        from . import append as appendmod
        self._prefill_entry("prefill_shared")
        cfg, B, dev = self.cfg, self.B, self.dev
        self._single_gpu("prefill_shared")
        assert self.pager is None, \
            "prefill_shared: the engine runs over a page pool - the aliased prefix pages would be released once per row that names them, " \
            "and the pool keeps no reference counts; prefill_chunked, or an engine without page_pool"
        assert not self._lora, \
            "prefill_shared: LoRA is on (set_lora) - a shared prefix under different adapters has different K / V, so its pages cannot " \
            "be computed once for the batch; set_lora(None), or prefill_chunked"
        prefix_tokens, suffix_tokens = prefix_tokens.to(dev), suffix_tokens.to(dev)
        assert prefix_tokens.dim() == 1 and suffix_tokens.dim() == 2 and suffix_tokens.size(0) == B and suffix_tokens.size(1) >= 1, \
            "prefill_shared: prefix_tokens [P], suffix_tokens [B, S] with S >= 1"
        P, S = prefix_tokens.numel(), suffix_tokens.size(1)
        P64 = 64 * (P // 64)
        own = torch.cat([prefix_tokens[P64:].unsqueeze(0).expand(B, -1), suffix_tokens], dim=1)      # [B, R]: what every sequence runs itself
        R = own.size(1)
        assert P + S + 1 <= self.max_len and (chunk is None or chunk >= 1)
        chunk = max(P64, R) if chunk is None else min(chunk, max(P64, R))
        bufs = self._prompt_buffers(max(B * min(chunk, R), min(chunk, P64)))
        # 1. the whole pages of the prefix, once, through row 0 of the tables
        self._prompt_pass(prefix_tokens[:P64].unsqueeze(0), [P64], chunk, bufs, 0, self._append_over([t[0:1] for t in self.tables]))
        # 2. every sequence names sequence 0's prefix pages
        for t in self.tables:
            t[:, :, :P64 // 64] = t[0:1, :, :P64 // 64]
        # 3. the rest of every prompt, the shared pages read once for the batch
        groups = appendmod.shared_prefix_groups([B], [P64], dev, batch=B)

        def attend_own(li, qkv, cu, past, n, c0, live):
            return appendmod.append_shared(qkv, cu, past, self.tables[li], self.H, self.Hkv, self.size_per_token, self.rope_base,
                                           self.int4, groups, max_seqlen_q=n, max_group_tokens=B * n, max_prefix=P64, max_suffix_past=c0)

        self._prompt_head(self._prompt_pass(own, [R] * B, chunk, bufs, P64, attend_own), P + S)

    # ---- verification of a draft tree (no reference counterpart; qserve_amd.append, csrc/append_tree.hip) ---------------------
    def verify_tree(self, draft_tokens, parents, device_walk=False, sampled=False):
        """Verify one draft tree per sequence in ONE pass and keep the greedy path.  `parents` [n] (n <= 64, the same tree shape for
        every sequence): parents[i] is the parent of node i, an EARLIER node; node 0 is the root - the current `tokens`, whose K / V
        are not in the cache yet - and parents[0] = -1.  `draft_tokens` int64 [B, n]: the drafted token of every node (column 0 is
        replaced by `tokens`).

        The B * n rows run through the is_prompt layer stack with `append_tree` at past = lengths - 1: node i is rotated at position
        past + depth(i), sees the context and its ancestors, and parks its K / V in slot past + i.  Then logits and argmax for all
        rows, and per sequence the greedy walk: from the root, descend to the (first) child whose token equals its parent's argmax,
        until none matches.  `commit_path` moves the accepted nodes' K / V to slots past .. past + m - 1 of every layer; `tokens`
        becomes the argmax at the last accepted node, `lengths` grow by m - the state m decode steps would have left, so step() /
        capture() / run() and a further verify_tree (now with ragged lengths) go on from here.  The slots behind the path keep the
        rejected nodes' bytes: readers mask them by `lengths`, the next writer overwrites them.
        -> (accept_idx int32 [B, n] - node indices of the path, the first accept_lens[b] of a row are valid -, accept_lens int32 [B],
        argmax int64 [B, n]), on the device.

        `device_walk=True`: the same call with nothing leaving the device after the argument checks - no read-back, no host-built
        tensor.  The walk is `append.accept_greedy`, the commit ONE `append.commit_path_layers` launch for all layers, the last accepted
        rows are gathered by index; masks, cu_seqlens, the parents array and the table of layer tables come from a cache keyed by the
        parent tuple.  The planner hint and the "fits the page tables" bound are the engine's host-side upper bound of `lengths`, which
        such a call can only advance by n (sync_length_bound() tightens it).  Same triple and same state as the host path - bit for bit
        wherever both hints give the same split plan (the merge of split-KV partial results rounds differently from the un-split
        sum); it can be captured (capture_verify / run_verify).

        `sampled=True` (after set_sampling; both paths): lossless speculative sampling for point proposals.  The B * n rows are sampled in
        one `sampling.sample_rows` launch, node i of sequence b keyed by (b, lengths[b] - 1 + depth(i) + 1) - the position of the token
        that FOLLOWS the node - and the sampled tokens take the place of the arg-max in the walk: descend to the child that carries the
        token drawn at its parent, else that token is the bonus token.  (Siblings' subtrees share keys at equal depth; one path is
        walked.)  Commit, `tokens`, `lengths` as above; the third element of the triple is the sampled tokens."""
        from . import append as appendmod
        B, dev = self.B, self.dev
        par = self._tree_arg(parents, "verify_tree", drafting=False)
        n = len(par)
        assert tuple(draft_tokens.shape) == (B, n) and draft_tokens.dtype == torch.int64
        self._sampled_entry("verify_tree", sampled)
        if device_walk:
            return self._verify_tree_device(draft_tokens, par, sampled=sampled)
        self._host_walk_entry()
        max_past = int(self.lengths.max()) - 1
        self._fits("verify_tree", n, max_past)
        self._reserve(n)
        _, toks, past, h, final, logits, am = self._verify_forward(draft_tokens, par, max_past, sampled)
        am = am.view(B, n)
        # the greedy walk, on the host (n <= 64 nodes per sequence)
        am_h, tok_h = am.cpu().tolist(), toks.cpu().tolist()
        kids = [[c for c in range(1, n) if par[c] == i] for i in range(n)]
        idx_h, len_h = [], []
        for b in range(B):
            path, cur = [0], 0
            while True:
                nxt = next((c for c in kids[cur] if tok_h[b][c] == am_h[b][cur]), None)
                if nxt is None:
                    break
                path.append(nxt)
                cur = nxt
            len_h.append(len(path))
            idx_h.append(path + [0] * (n - len(path)))
        accept_idx = torch.tensor(idx_h, dtype=torch.int32, device=dev)
        accept_lens = torch.tensor(len_h, dtype=torch.int32, device=dev)
        for li in range(len(self.layers)):
            appendmod.commit_path(self.tables[li], past, accept_idx, accept_lens, self.Hkv, self.size_per_token, self.int4)
        last = torch.tensor([b * n + idx_h[b][len_h[b] - 1] for b in range(B)], dtype=torch.int64, device=dev)
        self.hidden.copy_(torch.index_select(h, 0, last))
        self.final.copy_(torch.index_select(final, 0, last))
        self.tokens.copy_(torch.index_select(am.reshape(-1), 0, last))      # in place: captured graphs read these tensors
        self.lengths.add_(accept_lens)
        self._len_bound = max_past + 1 + max(len_h)                         # (tight again: both are known on the host)
        self.last_verify_logits = logits.view(B, n, -1)                     # (kept for callers that sample or score themselves)
        return accept_idx, accept_lens, am

    def sync_length_bound(self):
        """Make the host-side upper bound of `lengths` exact again (one device read-back): device-walk verifications advance it by the
        tree's n nodes each, whatever was accepted."""
        self._len_bound = int(self.lengths.max())
        return self._len_bound

    def _sampled_entry(self, what, sampled):
        """What every entry with a `sampled` argument asks for before it samples."""
        assert not sampled or self.sampling is not None, f"{what}(sampled=True): set_sampling first"

    def _host_walk_entry(self):
        """What verify_tree(device_walk=False) refuses: the features whose launches only the device walk issues."""
        for on, why in ((self.penalties, "penalties (set_penalties) need device_walk=True - the host walk does not penalise"),
                        (self.stopping, "stopping (set_stopping) needs device_walk=True - the host walk does not clip its path"),
                        (self._logprobs, "log-probabilities (set_logprobs) need device_walk=True - the host walk does not record them"),
                        (self._fsm, "a constraint (set_constraint) needs device_walk=True - the host walk does not advance its states")):
            assert on is None, f"verify_tree: {why}"

    def _fits(self, what, n, max_past=None):
        """Do n more slots behind `max_past` fit the page tables?  None: behind the host-side bound of the lengths."""
        by_bound = max_past is None
        assert (self._len_bound - 1 if by_bound else max_past) + n <= self.mb * 64, \
            f"{what}: the tree does not fit the sequences' page tables" + \
            (" (by the host-side bound of the lengths: sync_length_bound())" if by_bound else "")

    def _tree_constants(self, par):
        """The device tensors a verification or a drafter needs for the tree `par` (built on the host once, then served from the cache)."""
        from . import append as appendmod
        key = tuple(par)
        c = self._tree_cache.get(key)
        if c is None:
            B, n, dev = self.B, len(par), self.dev
            if self._layer_tables is None:
                self._layer_tables = appendmod.layer_table_pointers(self.tables)
            if len(self._tree_cache) >= 16:              # (a serving loop uses a handful of tree shapes)
                self._tree_cache.pop(next(iter(self._tree_cache)))
            c = dict(masks=appendmod.tree_masks_from_parents(par * B, [i * n for i in range(B + 1)]).to(dev),
                     cu=torch.arange(0, B + 1, device=dev, dtype=torch.int32) * n,
                     parents=torch.tensor(par * B, dtype=torch.int32, device=dev), layer_tables=self._layer_tables,
                     tree=torch.tensor(par, dtype=torch.int32, device=dev),          # [n]: the one tree shape the drafter takes
                     depth=torch.tensor(_tree_depths(par), dtype=torch.int32, device=dev))
            self._tree_cache[key] = c
        return c

    def _node_keys(self, depth):
        """The keys of the B * n rows of a sampled verification: node i of sequence b draws the token at position lengths[b] + depth(i)."""
        n = depth.numel()
        return samplingmod.position_keys(self._samp_ids.view(-1, 1).expand(self.B, n), self.lengths.view(-1, 1) + depth.view(1, -1)).reshape(-1)

    def _verify_forward(self, draft_tokens, par, max_past, sampled):
        """The forward pass of a verification, the same for both walks: the roots take the place of column 0 of the draft, the B * n
        rows run through the layer stack with `append_tree` at past = lengths - 1 (`max_past`: the planner hint), then norm and head
        (penalised while set_penalties is on - the lengths have not advanced yet -, sampled under the node keys with `sampled`).
        Nothing leaves the device.  -> (the tree's constants, tokens [B, n], past, hidden rows, normed rows, logits, the head's tokens
        [B * n])."""
        from . import append as appendmod
        cfg, B, dev, n = self.cfg, self.B, self.dev, len(par)
        c = self._tree_constants(par)
        cu, masks = c["cu"], c["masks"]
        toks = draft_tokens.to(dev).clone(memory_format=torch.contiguous_format)
        toks[:, 0] = self.tokens
        past = self.lengths - 1
        h = torch.index_select(self.embed, 0, toks.reshape(-1))

        def attend(li, qkv):
            return appendmod.append_tree(qkv, cu, past, self.tables[li], masks, self.H, self.Hkv, self.size_per_token,
                                         self.rope_base, self.int4, max_seqlen_q=n, max_past=max_past).reshape(B * n, -1)

        self._prompt_layers(h, self._prompt_buffers(B * n), attend)
        final = torch.empty_like(h)
        layernorm_ops.rms_norm(final, h, self.norm_w, cfg["eps"])
        am = torch.empty((B * n,), dtype=torch.int64, device=dev)
        logits = self._head(final, am, (lambda: self._node_keys(c["depth"])) if sampled else None, draft=(toks, c["tree"]))
        return c, toks, past, h, final, logits, am

    def _verify_tree_device(self, draft_tokens, par, max_past=None, out=None, sampled=False, reserved=False):
        """verify_tree(device_walk=True) behind its argument checks.  `max_past`: the planner hint (None: the host-side bound);
        `out`: accept_greedy's four output tensors (None: fresh ones); `reserved`: the caller's round began with the pool's reserve."""
        from . import append as appendmod
        B, n = self.B, len(par)
        self._fits("verify_tree", n)
        if not reserved:
            self._reserve(n)
        hint = self._len_bound - 1 if max_past is None else int(max_past)
        c, toks, past, h, final, logits, am = self._verify_forward(draft_tokens, par, hint, sampled)
        accept_idx, accept_lens, last, nxt = appendmod.accept_greedy(toks.view(-1), am, c["parents"], c["cu"], max_accept=n, out=out)
        self._emit(logits, nxt, node_tokens=toks, accept_idx=accept_idx, accept_lens=accept_lens, last_row=last)
        appendmod.commit_path_layers(c["layer_tables"], past, accept_idx, accept_lens, self.mb, self.Hkv, self.size_per_token, self.int4)
        self.hidden.copy_(torch.index_select(h, 0, last))
        self.final.copy_(torch.index_select(final, 0, last))
        self.tokens.copy_(nxt)                                              # in place: captured graphs read these tensors
        self.lengths.add_(accept_lens)
        self._len_bound += n
        self.last_verify_logits = logits.view(B, n, -1)                     # (penalised / masked, while set_penalties / set_constraint is on)
        return accept_idx, accept_lens, am.view(B, n)

    def _capture_round(self, what, par, fn, max_past, sampled):
        """capture_verify / capture_speculate behind `_tree_arg`: capture fn - _verify_tree_device or _speculate - over a persistent
        [B, n] draft buffer and persistent (accept_idx, accept_lens, last_row, next_token) outputs of the walk -> the record.  Kept: those
        buffers (two of the outputs are not part of the result) and the tree's constants, which the cache may evict."""
        self._sampled_entry(what, sampled)
        n, B, dev = len(par), self.B, self.dev
        hint = self.max_len if max_past is None else int(max_past)
        draft = torch.zeros((B, n), dtype=torch.int64, device=dev)
        out = (torch.zeros((B, n), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
               torch.zeros((B,), dtype=torch.int64, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev))
        captured = self._capture(lambda: fn(draft, par, max_past=hint, out=out, sampled=sampled), n)
        return self._captured(captured, n, draft, out, self._tree_constants(par), tree=tuple(par), sampled=bool(sampled))

    def capture_verify(self, parents, max_past=None, sampled=False):
        """Capture one device-walk verify_tree of the tree `parents` in a hipGraph, the way capture() captures step() (`_capture`: a
        warm-up call first), over a persistent [B, n] draft buffer.  run_verify(draft_tokens) replays it.  `max_past`: the hint the split
        plan is frozen with (default: the engine's capacity, prompt_len + max_new); results never depend on it.  The warm-up is a real
        verification of an all-zero draft: it advances `tokens`, `lengths` and the cache like any other, so capture on a state you
        restore or do not care about - what capture() implies for step().  `sampled=True` captures verify_tree(sampled=True) (after
        set_sampling).  Single GPU, with the lm_head."""
        par = self._tree_arg(parents, "capture_verify", drafting=False)
        self._verify_capture = self._capture_round("capture_verify", par, self._verify_tree_device, max_past, sampled)
        self.verify_graph = self._verify_capture.graph
        return self.verify_graph

    def run_verify(self, draft_tokens):
        """Replay the verification capture_verify captured on `draft_tokens` int64 [B, n] -> the persistent (accept_idx, accept_lens,
        argmax) tensors of the capture (overwritten by the next replay)."""
        assert self.verify_graph is not None, "run_verify: capture_verify first"
        cap = self._verify_capture
        assert tuple(draft_tokens.shape) == (self.B, cap.n) and draft_tokens.dtype == torch.int64
        self._fits("run_verify", cap.n)
        cap.keep[0][0].copy_(draft_tokens)                                  # (the capture's draft buffer)
        self.verify_graph.replay()
        self._len_bound += cap.n
        return cap.result

    # ---- n-gram drafting and the closed speculative loop (qserve_amd.drafting, csrc/ngram_draft.hip) -----------------------------
    def enable_drafting(self, prompt_tokens, max_ngram=4, min_match=1, pad_token=0):
        """Start keeping the text of every sequence on the device, for the n-gram drafter: `history` int32 [B, max_len], columns
        0 .. P - 1 the prompt (`prompt_tokens`: what the prefill entry was given, [B * P] sequence-major or [B, P]), column P the first
        sampled token (`tokens`) - history[b, :lengths[b]] is the text, its last entry the token whose K / V is not in the cache yet.
        Call it right after a prefill entry that was given `tokens` (all sequences hold P + 1 tokens: checked, one read-back).  From
        then on step() records history[b, lengths[b] - 1] = tokens[b] behind its head (one more launch pair; a graph captured AFTER
        this call contains it, one captured before does not record) and speculate() records what it accepted.  verify_tree() itself
        does not touch `history`: a caller that verifies drafts of its own appends with drafting.history_append.  `max_ngram`,
        `min_match`: the drafter's parameters (drafting.ngram_draft_tree) from now on.  `pad_token`: what a node without a candidate
        holds - the verification embeds every node, so it must be a token of the vocabulary (0 <= pad_token < vocab; checked).  A
        second call (after another prefill) refills the SAME buffers in place: graphs captured since the first call stay valid.
        `prompt_lens` int32 [B] holds P, where the generated text begins (what set_penalties counts as generated); refilled as well.
        `prompt_tokens=None`: the history of an EMPTY batch, after no prefill at all - lengths = 1, prompt_lens = 0, under a page pool
        every row's pages released; a set_stopping(stop, 0) behind it freezes every row by the at-the-limit rule.  That is the state
        admit() fills row by row and serve() starts from.  Single GPU, with the lm_head."""
        self._single_gpu("enable_drafting")
        assert 1 <= int(min_match) <= int(max_ngram) <= draftingmod.MAX_NGRAM, \
            f"enable_drafting: 1 <= min_match <= max_ngram <= {draftingmod.MAX_NGRAM}"
        assert 0 <= int(pad_token) < self.cfg["vocab"], \
            f"enable_drafting: pad_token={int(pad_token)} must be a token of the vocabulary (0 .. {self.cfg['vocab'] - 1}): pad nodes are embedded"
        B, dev = self.B, self.dev
        if prompt_tokens is None:
            # the empty batch: every row a text of one token (whatever `tokens` holds) that nobody asked for, lengths = 1, prompt_lens = 0,
            # no page owned - a set_stopping(stop, 0) behind it freezes every row at its limit: what admit() fills and serve() starts from
            prompt, P = None, 0
            if self.pager is not None:
                self.release_rows(None)
            self.lengths.fill_(1)
            self._len_bound, self._text_start = 1, 0
        else:
            prompt = prompt_tokens.to(dev).reshape(B, -1)
            P = prompt.size(1)
            assert P + 1 <= self.max_len and bool((self.lengths == P + 1).all()), \
                "enable_drafting: call it right after a prefill of these prompt tokens (every sequence holds P + 1 tokens)"
        if self.history is None:
            self.history = torch.zeros((B, self.max_len), dtype=torch.int32, device=dev)
            # what history_append needs to record ONE token per sequence (a path of the root alone): constants of step()'s record,
            # and the buffer its `past` is computed into
            self._step_record = (torch.zeros((B, 1), dtype=torch.int64, device=dev), torch.zeros((B, 1), dtype=torch.int32, device=dev),
                                 torch.ones((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
            self.prompt_lens = torch.zeros((B,), dtype=torch.int32, device=dev)   # P: where the generated text begins (set_penalties)
        self.history.zero_()
        self.prompt_lens.fill_(P)
        self._prompt_len = P                                                  # (the same value on the host, for set_stopping's limits)
        self._text_starts = None                                              # (admit: `prompt_lens` on the host, once rows differ)
        if prompt is not None:
            self.history[:, :P] = prompt
        self.history[:, P] = self.tokens
        self._draft_params = (int(max_ngram), int(min_match), int(pad_token))

    # ---- repetition, presence and frequency penalties (qserve_amd.penalties, csrc/penalize_rows.hip) ----------------------------
    def set_penalties(self, repetition=1.0, frequency=0.0, presence=0.0):
        """Penalise the logits in front of every head that reads `history` (after enable_drafting): one `penalties.penalize_rows` launch
        directly in front of the arg-max / the sampler of step() (hence capture() / run()) - context: the text history[b, :lengths[b]] -
        and of verify_tree(device_walk=True) (hence capture_verify, speculate, capture_speculate) - context of node i: the text plus the
        drafted tokens on the path to i, what a plain step() would see at that position if the path is accepted, so the generated tokens
        still do not depend on what was drafted.  Greedy heads are penalised too.  x = x / repetition if x > 0 else x * repetition for
        every token of the context; then x -= frequency * c + presence * (c > 0), c = the token's occurrences behind the prompt (the P
        of enable_drafting).  set_penalties(None) switches it off: every path launches exactly what it launches without this call.
        The three values live in persistent float32 [B] device tensors that are filled in place, so a captured graph sees later changes
        of them; whether the launch exists at all is frozen into a capture - capture after switching.  `last_verify_logits` holds the
        PENALISED logits while on.  Limits: the first token of a sequence is drawn by the prefill head, unpenalised (a prefill entry
        refuses to run while penalties are on); the host-walk verify_tree(device_walk=False) refuses too; single GPU, with the lm_head;
        the history's capacity prompt_len + max_new must not exceed 65 472 (16-bit counts)."""
        if repetition is None:
            self.penalties = None
            return
        self._single_gpu("set_penalties")
        assert self.history is not None, "set_penalties: enable_drafting first (the penalties read `history`)"
        assert self.history.size(1) <= penaltiesmod.MAX_CAP, \
            f"set_penalties: the history holds {self.history.size(1)} tokens per sequence, the penalty counts at most {penaltiesmod.MAX_CAP}"
        assert self.cfg["vocab"] >= 8 and self.cfg["vocab"] % 8 == 0, "set_penalties: the logit rows need a vocabulary that is a multiple of 8"
        assert float(repetition) > 0.0, f"set_penalties: repetition={float(repetition)} must be > 0"
        if self._pen_values is None:
            self._pen_values = tuple(torch.empty((self.B,), dtype=torch.float32, device=self.dev) for _ in range(3))
        for t, v in zip(self._pen_values, (repetition, frequency, presence)):
            t.fill_(float(v))
        self.penalties = self._pen_values

    def _penalize(self, logits, node_tokens=None, tree=None):
        """The launch in front of a head: `logits` [B * n, V] in place, from `history`, the lengths as they stand and the draft."""
        rep, freq, pres = self.penalties
        penaltiesmod.penalize_rows(logits, self.history, self.lengths, self.prompt_lens, node_tokens, tree, rep, freq, pres)

    # ---- stop conditions (qserve_amd.stopping, csrc/stop_update.hip) -----------------------------------------------------------
    def set_stopping(self, stop=(), max_new_tokens=None):
        """End sequences on the device (after enable_drafting: the rule reads `history` and `prompt_lens`): one `stopping.stop_update`
        launch in the tail of every round (`_emit` has where, and the order).  `stop`: token ids and / or sequences of ids (at most 32 of at most 8 tokens);
        a sequence ends with the token that completes one of them INSIDE its generated text (a match may not begin in the prompt).
        `max_new_tokens`: an int, or one per sequence - a sequence ends when its text holds prompt + max_new_tokens tokens; None: the
        history's capacity (prompt_len + max_new of the engine), which an explicit value must not exceed.  A round's path is clipped at
        the first stop, so a sequence's text is the text of an engine without stopping, cut there - and nothing of another sequence changes.
        `finished` int32 [B] holds why: 0 live, 1 a stop sequence, 2 the length.

        A finished sequence is FROZEN, inside the fixed batch: its `tokens`, `lengths` and `history[b, :lengths[b]]` never change again;
        its page slots < lengths[b] keep their bytes (a frozen step() rewrites slot lengths[b] - 1 with the same token at the same
        position, a frozen verification parks its nodes in slots >= lengths[b] - 1 and commits none); its rows of `hidden` and `final`
        are unspecified.  Its row still runs through every GEMM - the batch is fixed under a graph and is not compacted.

        Table, limits and `finished` live in persistent device tensors that are filled in place: a captured graph sees a later
        set_stopping(...) with new values; whether the launch exists at all is frozen into a capture - capture after switching.  The
        call clears `finished` and looks at the current token once (the token a prefill head drew): a sequence whose first token is
        already a stop, or that is already at its limit, is finished at once.  set_stopping(None) switches it off: every path launches
        exactly what it launches without this call.  The prefill entries and the host-walk verify_tree(device_walk=False) refuse to run
        while it is on.  Single GPU, with the lm_head."""
        if stop is None:
            self.stopping = None
            return
        self._single_gpu("set_stopping")
        assert self.history is not None, "set_stopping: enable_drafting first (the stop rule reads `history`)"
        B, dev, cap = self.B, self.dev, self.history.size(1)
        seqs, lens = stoppingmod.stop_table(stop, num_rows=stoppingmod.MAX_STOPS, width=stoppingmod.MAX_STOP_LEN)
        if max_new_tokens is None:
            limits = [cap] * B
        else:
            new = [int(max_new_tokens)] * B if isinstance(max_new_tokens, int) else [int(v) for v in max_new_tokens]
            assert len(new) == B and min(new) >= 0, f"set_stopping: max_new_tokens is one non-negative int, or one per sequence ({B})"
            limits = [p + v for p, v in zip(self._row_starts(), new)]
            assert max(limits) <= cap, \
                f"set_stopping: text start + max_new_tokens {limits} is beyond the history's capacity {cap}"
        if self.finished is None:
            self.finished = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.limit_lens = torch.zeros((B,), dtype=torch.int32, device=dev)
            self._stop_seqs, self._stop_lens = torch.empty_like(seqs, device=dev), torch.empty_like(lens, device=dev)
            self._stop_k = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._stop_seqs.copy_(seqs)
        self._stop_lens.copy_(lens)
        self.limit_lens.copy_(torch.tensor(limits, dtype=torch.int32))
        self.finished.zero_()
        self.stopping = True
        self._stop_k.zero_()                                                # m = 0: nothing is emitted, the current token is looked at
        self._stop_update(self.tokens, accept_lens=self._stop_k, check_root=True)

    def _stop_update(self, next_token, **path):
        """The launch of set_stopping's rule on what a round is about to emit, from `history` and the lengths as they stand (not yet
        advanced) -> k int32 [B]."""
        return stoppingmod.stop_update(self.history, self.lengths, next_token, self.finished, self._stop_seqs, self._stop_lens, self.limit_lens,
                                       self.prompt_lens, **path)

    # ---- log-probabilities (qserve_amd.logprobs, csrc/logprob_rows.hip) ---------------------------------------------------------
    def set_logprobs(self, top=0, tempered=False):
        """Record, for every token the engine emits from now on, its log-probability, its rank and the `top` (0 .. 32) most likely ids
        with their log-probabilities, on the device: one `logprobs.logprob_path` launch in the tail of every round (`_emit` has where,
        and the order: a clipped path records exactly what it emits and a frozen row records nothing) - in a verification the kernel
        itself gathers the rows on the accepted path and the token each is scored for -, and in the head of a prefill entry, whose token
        lands at column prompt_len (a prefill entry also clears the logs: a new text begins).  The logs, indexed by text position like `history`:
        `logprob_log` float32 [B, max_len] (NaN where nothing was recorded), `rank_log` int32 [B, max_len] (0), `top_ids_log` int32
        [B, max_len, top] (-1) and `top_lp_log` float32 [B, max_len, top] (NaN); logprobs() reads them.  The values describe
        softmax(logits / T) of the logits the head saw - penalised while set_penalties is on; top-k and top-p do not enter - with T = 1,
        or with `tempered` the temperature of set_sampling (which must be on; < 1e-5, the greedy setting, counts as 1).
        include/qserve_amd.h (`qs_logprob_rows`) has the arithmetic.

        The call clears the logs.  They are persistent device tensors (re-created only for another `top`); whether the launch exists,
        `top` and `tempered` are frozen into a capture - capture after switching; generate() re-captures by itself.
        set_logprobs(None) switches it off: every path launches exactly what it launches without this call.  The host-walk
        verify_tree(device_walk=False) refuses to run while it is on.  Single GPU, with the lm_head."""
        if top is None:
            self._logprobs = None
            return
        self._no_beams("set_logprobs", "the logs are indexed by row and text position and do not follow a regroup (`beam_score` is the sum)")
        self._single_gpu("set_logprobs")
        top = int(top)
        assert 0 <= top <= logprobsmod.MAX_TOP, f"set_logprobs: top={top} (0 .. {logprobsmod.MAX_TOP})"
        assert self.cfg["vocab"] >= 8 and self.cfg["vocab"] % 8 == 0, "set_logprobs: the logit rows need a vocabulary that is a multiple of 8"
        assert not tempered or self.sampling is not None, "set_logprobs(tempered=True): set_sampling first (its temperature is the one used)"
        if self.logprob_log is None or self.top_ids_log.size(2) != top:
            self.logprob_log, self.rank_log, self.top_ids_log, self.top_lp_log = logprobsmod.new_logs(self.B, self.max_len, top, self.dev)
        self._logprobs = (top, bool(tempered))
        self._clear_logprob_logs()

    def _clear_logprob_logs(self, rows=None):
        """Empty the logs of the rows `rows` (int64 indices; None: of every row)."""
        for log, empty in ((self.logprob_log, float("nan")), (self.rank_log, 0), (self.top_ids_log, -1), (self.top_lp_log, float("nan"))):
            log[slice(None) if rows is None else rows] = empty

    def logprobs(self):
        """Read the logs of set_logprobs once -> per sequence a dict of lists over its generated text, positions prompt_len ..
        lengths[b] - 1 - entry i belongs to token i of generate()'s texts, the first token of the prefill included (NaN / 0 where nothing
        was recorded, e.g. for a prefill that ran before set_logprobs): "logprobs" floats, "ranks" ints, "top_ids" / "top_logprobs"
        lists of `top` entries each."""
        assert self.logprob_log is not None, "logprobs: set_logprobs first"
        assert self._text_start is not None, "logprobs: after a prefill entry (it says where the generated text begins)"
        lens = self.lengths.cpu().tolist()
        lp, rank, ids, tlp = (t.cpu() for t in (self.logprob_log, self.rank_log, self.top_ids_log, self.top_lp_log))
        starts, res = self._text_starts or [self._text_start] * self.B, []   # (per row once admit has been used)
        for b in range(self.B):
            P, end = starts[b], min(lens[b], self.max_len)
            res.append(dict(logprobs=lp[b, P:end].tolist(), ranks=rank[b, P:end].tolist(), top_ids=ids[b, P:end].tolist(),
                            top_logprobs=tlp[b, P:end].tolist()))
        return res

    # ---- constrained decoding (qserve_amd.constraints, csrc/constrain_rows.hip) ---------------------------------------------------
    def set_constraint(self, dfa, start_states=0):
        """Restrict what every sequence may emit to the language of a token automaton (`constraints.TokenDFA`, on the host or on the
        device), on the device: `fsm_state` int32 [B] holds the automaton state of every sequence - `start_states` now: an int, or one per
        sequence, -1 for a sequence that stays unconstrained (several grammars in one batch: `TokenDFA.union` and its offsets).  From
        then on every head masks its rows in place, behind the penalty launch and in front of the arg-max / the sampler
        (`constraints.constrain_rows`: -inf wherever the row's state does not allow the token): step() (hence capture() / run()) and the
        head of a prefill entry under `fsm_state`, verify_tree(device_walk=True) (hence capture_verify, speculate, capture_speculate)
        every row under the state of its own node, the state reached along the path root -> node (`constraints.node_states`, launched
        just before).  A child is accepted only if it holds the token its parent's masked row produced, so greedy and sampled
        speculation stay lossless: the generated tokens are those of constrained step()s, whatever was drafted.  `constraints.advance`
        then moves `fsm_state` over what the round emitted, in its tail (`_emit` has where, and the order); a frozen row keeps its state.
        The logits a head returns, `last_verify_logits` and what set_logprobs scores are the MASKED ones.

        A state the automaton has no way out of for the token emitted becomes constraints.DEAD (-2) - it cannot happen through the
        engine's own heads unless a state allows no token at all - and a dead or negative state is unconstrained.  Unlike penalties and
        stopping the constraint needs no `history`: the prefill entries run while it is on, mask the first token with the start states
        and advance once - so call set_constraint (again) BEFORE every prefill: `fsm_state` is where the last text left it.

        `fsm_state` and the node states live in persistent device tensors; `fsm_state` is filled in place, so a captured graph sees new
        start states.  The tables, and whether the launches exist at all, are frozen into a capture - capture after switching;
        generate() re-captures by itself.  Calling it again with the SAME TokenDFA object keeps the tables (and every capture made with
        them) and only refills the states - also across a set_constraint(None) in between: the uploaded tables of the last automaton are
        kept, and a capture made with them is used again unless the graph was captured anew while the constraint was off.
        set_constraint(None) switches it off: every path launches exactly what it launches without this call.  The host-walk verify_tree(device_walk=False) refuses to run while it is on.  Single GPU, with the lm_head; the
        vocabulary must be a multiple of 8 and equal dfa.token_class.numel()."""
        if dfa is None:
            self._fsm = None                                 # (the uploaded tables stay in _fsm_kept, for the same object's return)
            return
        self._single_gpu("set_constraint")
        from .append import MAX_TREE
        B, V = self.B, self.cfg["vocab"]
        assert isinstance(dfa, constraintsmod.TokenDFA), "set_constraint: a constraints.TokenDFA (or None)"
        assert V >= 8 and V % 8 == 0, "set_constraint: the logit rows need a vocabulary that is a multiple of 8"
        assert dfa.V == V, f"set_constraint: the automaton names {dfa.V} tokens, the vocabulary has {V}"
        start_states = torch.as_tensor(start_states, device="cpu")          # (a Python or numpy integer, a sequence, an array, a tensor)
        assert start_states.dim() <= 1 and not start_states.is_floating_point() and start_states.dtype != torch.bool, \
            f"set_constraint: start_states is one int, or one int per sequence ({B}), got {start_states.dtype} {tuple(start_states.shape)}"
        starts = [int(start_states)] * B if start_states.dim() == 0 else [int(v) for v in start_states]
        assert len(starts) == B, f"set_constraint: start_states is one int, or one per sequence ({B})"
        if self.fsm_state is None:
            self.fsm_state = torch.full((B,), -1, dtype=torch.int32, device=self.dev)
            self._fsm_node_state = torch.full((B * MAX_TREE,), -1, dtype=torch.int32, device=self.dev)
        self.fsm_state.copy_(torch.tensor(starts, dtype=torch.int32))
        if self._fsm_src is not dfa:
            d = dfa.to(self.dev)
            self._fsm_kept, self._fsm_src = (d.token_class, d.next), dfa
        self._fsm = self._fsm_kept

    def _constrain(self, logits, node_tokens=None, tree=None):
        """The mask launch in front of a head: `logits` [B * n, V] in place, the rows of a draft under their nodes' states."""
        token_class, nxt = self._fsm
        states = self.fsm_state
        if node_tokens is not None:
            states = self._fsm_node_state[:node_tokens.numel()]
            constraintsmod.node_states(self.fsm_state, node_tokens, tree, token_class, nxt, out=states)
        constraintsmod.constrain_rows(logits, states, token_class, nxt)

    # ---- LoRA adapters (qserve_amd.lora, csrc/lora_rows.hip) -----------------------------------------------------------------------
    def enable_lora(self, slots, rank):
        """Create the adapter table: `slots` adapters of rank <= `rank` (8, 16, 32 or 64) for the four linears of every layer
        (`lora.LoraTable`, zeroed), and `lora_ids` int32 [B], every sequence at -1.  Nothing runs differently until set_lora.  A second
        call makes a new table and switches LoRA off; a graph captured with the old one keeps reading the old one.  Single GPU, with
        the lm_head."""
        self._single_gpu("enable_lora")
        assert self.moe is None, "enable_lora: LoRA over expert weights is not built - a mixture-of-experts engine runs the base model only"
        self.lora_table = loramod.LoraTable(self.cfg, slots, rank, self.dev)
        self.lora_ids = torch.full((self.B,), -1, dtype=torch.int32, device=self.dev)
        ws = max(loramod.workspace_bytes(self.B, K, self.lora_table.rank, len(ends)) for K, _, ends in self.lora_table.shapes.values())
        self._lora_step_ws = torch.empty((max(ws, 16),), dtype=torch.uint8, device=self.dev)
        self._lora = False

    def load_lora(self, slot, tensors, alpha):
        """`lora.LoraTable.load`: fill `slot` from a dict of PEFT-named lora_A / lora_B tensors, scaling = alpha / r'.  In place: a captured
        graph sees the new adapter."""
        assert self.lora_table is not None, "load_lora: enable_lora first"
        self.lora_table.load(slot, tensors, alpha)

    def unload_lora(self, slot):
        """`lora.LoraTable.unload`: zero `slot` (sequences still pointing at it add exact zeros)."""
        assert self.lora_table is not None, "unload_lora: enable_lora first"
        self.lora_table.unload(slot)

    def set_lora(self, adapter_ids):
        """Run sequence b under adapter adapter_ids[b] (one int per sequence; -1, or any id outside 0 .. slots-1: the base model) from
        now on: one `lora.lora_rows` call behind each of the four base GEMMs of every layer (and behind its bias), on the quantised
        activations that GEMM read, on every path - step() (hence capture() / run()), prefill, prefill_chunked, verify_tree, speculate and
        their captures; rows_per_seq is the path's rows / B.  While on, the four linears take the path a linear with a bias takes: `o`
        and `down` run without the planes form, gate_up as the plain GEMM followed by silu_and_mul + quant - the same values, bit for bit,
        for a sequence at -1.  The ids live in `lora_ids`, filled in place: a captured graph sees later changes of them (and of the
        table's slots); whether the launches exist at all is frozen into a capture - capture after switching; generate() re-captures by
        itself.  set_lora(None) switches it off: every path launches exactly what it launches without this call.  prefill_shared refuses
        to run while it is on.  Single GPU, with the lm_head."""
        if adapter_ids is None:
            self._lora = False
            return
        self._single_gpu("set_lora")
        assert self.moe is None, "set_lora: LoRA over expert weights is not built - a mixture-of-experts engine runs the base model only"
        assert self.lora_table is not None, "set_lora: enable_lora first"
        ids = torch.as_tensor(adapter_ids, device="cpu")
        assert ids.dim() == 1 and ids.numel() == self.B and not ids.is_floating_point() and ids.dtype != torch.bool, \
            f"set_lora: one int per sequence ({self.B}), got {ids.dtype} {tuple(ids.shape)}"
        self.lora_ids.copy_(ids.to(torch.int32))
        self._lora = True

    def _lora_plan(self, rows, ids=None):
        """(adapter ids, rows_per_seq, workspace) of the lora_rows calls of a layer stack over `rows` rows: `lora_ids` with the step's
        persistent workspace, or with a fresh one sized for the largest of the four linears (inside a capture it lives in the graph's
        pool).  `ids`: the adapter of every TOKEN of a ragged pass int32 [rows] (rows_per_seq = 1); None: `lora_ids`, rows / B rows per
        sequence."""
        t, per_seq = self.lora_table, 1
        if ids is None:
            if rows == self.B:
                return self.lora_ids, 1, self._lora_step_ws
            per_seq, ids = rows // self.B, self.lora_ids
        assert ids.numel() * per_seq == rows
        ws = max(loramod.workspace_bytes(rows, K, t.rank, len(ends)) for K, _, ends in t.shapes.values())
        return ids, per_seq, torch.empty((max(ws, 16),), dtype=torch.uint8, device=self.dev)

    # ---- what the features share: the tail of a round, and what a capture freezes and keeps --------------------------------------
    def _emit(self, logits, next_token, node_tokens=None, accept_idx=None, accept_lens=None, last_row=None, lengths=None, k=None):
        """THE tail of a round, on what it is about to emit, at the lengths as they stand (not yet advanced): behind the head of step()
        (hence capture() / run()) and of a prefill entry (where stopping is off), between the walk and the commit of
        verify_tree(device_walk=True) (hence capture_verify, speculate, capture_speculate).  `logits`: the rows the head saw;
        `next_token`: the token behind the path; a verification adds its draft and the walk's outputs (`node_tokens` [B, n], `accept_idx`,
        `accept_lens`, `last_row`), the others give none: one token per sequence.  In this order, whatever is switched on:
          1. set_stopping: `stopping.stop_update` clips the path at the first stop, in place, -> k int32 [B] - `accept_lens` itself, or
             `_stop_k` (0 / 1) for a step; a finished row emits nothing;
          2. set_logprobs: `logprobs.logprob_path` scores the (clipped) path's rows, each for the token behind it - k = 0 writes nothing;
          3. set_constraint: `constraints.advance` moves `fsm_state` from the state of the (clipped) path's last row - under a draft its
             node's, of `_fsm_node_state` - over the token it emitted; k = 0 keeps the state.
        -> k while stopping is on (what the lengths advance by), else None.  The head of an admission (`_prompt_head` over some rows)
        hands over `k` - 1 on the admitted rows, 0 elsewhere - in place of step 1, and `lengths`, the position of every row's token."""
        if k is None:
            k = accept_lens
            if self.stopping is not None:
                k = self._stop_update(next_token, node_tokens=node_tokens, accept_idx=accept_idx, accept_lens=accept_lens, last_row=last_row,
                                      out_lens=self._stop_k if accept_lens is None else None)
        if self._logprobs is not None:
            top, tempered = self._logprobs
            logprobsmod.logprob_path(logits, node_tokens, accept_idx, k, next_token, self.lengths if lengths is None else lengths,
                                     temperature=self._samp_t[:self.B] if tempered else 1.0, top=top,
                                     out=(self.logprob_log, self.rank_log, self.top_ids_log, self.top_lp_log))
        if self._fsm is not None:
            node_state = None if node_tokens is None else self._fsm_node_state[:node_tokens.numel()].view_as(node_tokens)
            constraintsmod.advance(self.fsm_state, next_token, *self._fsm, node_state=node_state, accept_idx=accept_idx, accept_lens=k)
        return k if self.stopping is not None else None

    def _capture_state(self):
        """What a capture freezes besides its own arguments, and generate() compares: whether the stop launch exists, the state of
        set_logprobs, the automaton whose tables are on - set_constraint uploads them once per TokenDFA object, so the object stands for
        the tables and compares by identity -, whether the LoRA launches exist, the beam width (None: the step takes the arg-max).  (Frozen too, and not in it: whether the head samples or
        penalises.)"""
        return dict(stops=self.stopping is not None, logprobs=self._logprobs, automaton=None if self._fsm is None else self._fsm_src,
                    lora=self._lora, beams=self.beams)

    def _kept_tensors(self):
        """Every persistent tensor a captured graph may touch and a later call may replace, by feature (None while the feature is off)."""
        return dict(drafting=(self._step_record, self.history, self.prompt_lens), penalties=self.penalties,
                    stopping=None if self.stopping is None else (self.finished, self.limit_lens, self._stop_seqs, self._stop_lens, self._stop_k),
                    logprobs=None if self._logprobs is None else (self.logprob_log, self.rank_log, self.top_ids_log, self.top_lp_log,
                                                                  self._samp_t),
                    constraint=None if self._fsm is None else (self._fsm, self.fsm_state, self._fsm_node_state),
                    lora=(self.lora_table, self.lora_ids, self._lora_step_ws) if self._lora else None,
                    beams=None if self.beams is None else (self.beam_score, *vars(self._beam).values()))

    def _captured(self, captured, n, *buffers, **own):
        """The record of the graph `_capture` just returned as `captured`: `graph`; `result`: what the captured call returned, tensors
        the replays overwrite; `n`: what a replay adds to the bound of the lengths; `state`: _capture_state() now, with what else decides
        whether this is the graph generate() was asked for (`own`; a round: the tree and the head); `keep`: every tensor the graph touches
        that was allocated outside the capture - it stays referenced as long as the graph does -: the capture's own `buffers` (a round:
        the draft buffer first) and _kept_tensors()."""
        return SimpleNamespace(graph=captured[0], result=captured[1], n=n, state=dict(self._capture_state(), **own),
                               keep=(buffers, self._kept_tensors()))

    def _stale(self, cap, **own):
        """generate(): was the graph of the record `cap` made in another state than the engine is in now, or not for `own`?"""
        return cap.state != dict(self._capture_state(), **own)

    def generate(self, max_rounds, parents=None, poll_every=8, sampled=False):
        """Decode until every sequence has finished (after set_stopping), with the host looking at the device once per burst: replay
        the captured step graph - or, with `parents`, the captured speculate graph of that tree - `poll_every` times, then read
        (`finished`, `lengths`) back in one copy; that is the only host <-> device traffic of the loop.  `_len_bound` is set from it.
        Ends when no sequence is live, when `max_rounds` rounds are done, or when another round would not fit the page tables by the
        bound (a burst is shortened to what fits).  A graph that does not exist yet, or that was captured in another `_capture_state()`
        (for speculation also: of another tree or head), is captured first - the warm-up of capture() / capture_speculate() is a real
        round that is not counted.
        -> (texts: per sequence the list of generated tokens history[b, prompt_lens[b] : lengths[b]], the first token of the prefill
        included; reasons: `finished` as a list; rounds; read_backs) - the texts are read once, after the loop."""
        assert self.stopping is not None, "generate: set_stopping first (nothing else ends the loop)"
        assert max_rounds >= 0 and poll_every >= 1
        advance, run = self._round_graph("generate", parents, sampled)
        rounds = reads = 0
        while rounds < max_rounds:
            burst = self._burst(run, advance, min(poll_every, max_rounds - rounds))
            if burst < 1:
                break
            rounds += burst
            state = torch.stack((self.finished, self.lengths)).cpu()         # the one read-back of the burst
            reads += 1
            self._len_bound = int(state[1].max())
            if bool((state[0] != 0).all()):
                break
        hist, lens, fin = self.history.cpu(), self.lengths.cpu().tolist(), self.finished.cpu().tolist()
        starts = self._row_starts()
        texts = [hist[b, starts[b]:lens[b]].tolist() for b in range(self.B)]
        return texts, fin, rounds, reads

    def _round_graph(self, what, parents, sampled):
        """The graph generate() replays: the captured step - or, with `parents`, the captured speculate round of that tree -,
        captured first where it does not exist yet or was captured in another state -> (what a replay adds to the lengths at most, the
        call that replays it)."""
        if parents is None:
            if self.graph is None or self._stale(self._step_capture):
                self.capture(piecewise=False)
            return 1, self.run
        par = self._tree_arg(parents, what)
        if self.speculate_graph is None or self._stale(self._speculate_capture, tree=tuple(par), sampled=bool(sampled)):
            self.capture_speculate(par, sampled=sampled)
        return len(par), self.run_speculate

    def _burst(self, run, advance, count):
        """Replay `run` up to `count` times, shortened to what fits the page tables by the host-side bound of the lengths -> the number
        of replays.  A round writes slots up to _len_bound - 1 + advance - 1."""
        burst = min(count, (self.mb * 64 - (self._len_bound - 1)) // advance)
        for _ in range(burst):
            run()
        return max(burst, 0)

    # ---- continuous batching: admission into rows of the fixed batch, and the loop over a stream of requests ----------------------
    def _row_starts(self):
        """Where every row's generated text begins, on the host: `prompt_lens`, per row once admit() has been used."""
        return self._text_starts or [self._prompt_len] * self.B

    def admit(self, rows, prompts, max_new_tokens=None, start_states=None, text_start=None, chunk=None, copy_rows=None):
        """Put new texts into the rows `rows` (distinct indices) of the fixed batch, eagerly, leaving every other row's `tokens`,
        `lengths`, `hidden`, `history`, logs, states and pages untouched byte for byte.  `prompts`: one 1-D token sequence per row,
        ragged, 1 <= P_r and P_r + 1 <= max_len.  After enable_drafting (enable_drafting(None) for an empty batch).  A static engine's
        rows keep their private pages; under a page pool the rows are released first and take the pages of their prompts' slots
        0 .. P_r - 1 in one reserve (lengths 1, extra_rows P_r, 0 elsewhere).  The caller sees to it that the free pages suffice
        (`pager.free_pages()`, or serve()'s bookkeeping): a refused row's prompt goes to the sink, and it ends with NO_PAGES while the stop
        rule is on (check() raises while it is off).

        The prompts, uploaded once, run through `_prompt_pass` in passes of `chunk` tokens per sequence (None: whole), `append.append`
        over the named rows' table rows - for equal-length prompts in every row the calls of prefill_chunked -, under set_lora with
        lora_ids[row] for every token of a row; `_prompt_head` over `rows` draws the first tokens, the constraint's mask under the
        row's `start_states` entry (an int or one per row; default 0; needs set_constraint to be on).  Then per row: history = the
        prompt and the first token behind zeros, prompt_lens = `text_start` (an int or one per row, 0 .. P_r; None: P_r - the text a
        resumed request generated earlier counts as generated), limit_lens = prompt_lens + `max_new_tokens` (an int or one per row;
        None: the history's capacity; needs set_stopping to have been called), finished = 0 followed by the root check of
        set_stopping while the stop rule is on.  Unlike the prefill entries it runs while stopping and penalties are on, and under
        set_lora.  No capture is invalidated.  Every argument is checked before the first write.  Single GPU, with the lm_head.

        Under a prefix cache (prefix_cache=True) the whole pages of a prompt's beginning that are cached, below its last token, are
        mapped into the row by one hold launch between the release and the reserve, the passes run tokens[c_r:] at past c_r + c0 only,
        and - behind one read-back of the rows' page ids - the floor(P_r / 64) whole pages the prompt filled are entered into the cache,
        which takes its holds in one more launch.  Requests of ONE admit do not share what none of them found cached.  admit never
        evicts (`evict_prefixes`).  Refused while set_lora is on.

        `copy_rows` (None, or per prompt a list of further rows; needs a counted pool): the FOLLOWERS start as further samples of the
        same prompt.  The rows named in `rows`, the leaders, run exactly what they run without it; then ONE fork launch pair maps the
        prompt's whole pages into the followers and copies the partly filled one (lengths P_r + 1: slot P_r is the first one a
        follower writes), and the head runs ONCE over leaders and followers, on the leaders' last hidden rows: every row draws its
        own first token under key (its row, P_r).  Texts, limits, states, adapters, cleared logs and the root check cover all of them.
        All rows, leaders and followers, must be distinct.

        Under set_beams every prompt starts one whole group: its leader is row g * W, its copy_rows the group's other rows in order.
        In place of the draw, `beams.select` runs over the head's rows with score 0 at the leaders and -inf at every other row: slot i of
        the group gets the leader's i-th best first token and its log-probability as `beam_score`.  All parents are the leader, whose
        copies the followers already are: nothing moves."""
        self._single_gpu("admit")
        assert self.prefix is None or not self._lora, \
            "admit: the engine has a prefix cache and LoRA is on (set_lora) - K / V under an adapter differ from the base model's, and a " \
            "slot can be reloaded under the same id, so its pages cannot be keyed by tokens alone; set_lora(None) before admitting"
        assert self.history is not None, "admit: enable_drafting first (enable_drafting(None) for an empty batch): it writes `history`"
        B, dev, cap = self.B, self.dev, self.max_len
        rows = [int(r) for r in rows]
        R = len(rows)
        assert R >= 1 and len(set(rows)) == R and all(0 <= r < B for r in rows), f"admit: rows {rows} - distinct row indices in 0 .. {B - 1}"
        lead = list(range(R))                                               # per row of `rows`: the index of the prompt it runs
        if copy_rows is not None:
            self._forkable("admit(copy_rows=)")
            copies = [[int(r) for r in c] for c in copy_rows]
            assert len(copies) == R, f"admit: copy_rows is one list of further rows per prompt ({R})"
            lead = lead + [i for i, c in enumerate(copies) for _ in c]
            rows = rows + [r for c in copies for r in c]
            assert len(set(rows)) == len(rows) and all(0 <= r < B for r in rows), \
                f"admit: rows and copy_rows {rows} - distinct row indices in 0 .. {B - 1} overall"
        if self.beams is not None:                                           # a prompt starts one whole group: its first tokens are the W best
            W = self.beams
            groups = [[r] + (copies[i] if copy_rows is not None else []) for i, r in enumerate(rows[:R])]
            assert all(g == list(range(g[0], g[0] + W)) and g[0] % W == 0 for g in groups), \
                f"admit: beam search is on (set_beams({W})) - every prompt starts one whole group: its row g * {W} in `rows`, the group's " \
                f"other rows, in order, as its copy_rows; got {groups}"
        pl = [torch.as_tensor(p).to("cpu", torch.int64) for p in prompts]
        assert len(pl) == R and all(p.dim() == 1 for p in pl), f"admit: one 1-D token sequence per row ({R})"
        Ps = [p.numel() for p in pl]
        assert min(Ps) >= 1 and max(Ps) + 1 <= cap, f"admit: prompt lengths {Ps} - 1 <= P and P + 1 <= max_len = {cap}"
        assert all(0 <= int(p.min()) and int(p.max()) < self.cfg["vocab"] for p in pl), "admit: a prompt token is outside the vocabulary"
        per_row = lambda v: [int(v)] * R if isinstance(v, int) else [int(x) for x in v]      # noqa: E731
        starts = Ps if text_start is None else per_row(text_start)
        assert len(starts) == R and all(0 <= s <= p for s, p in zip(starts, Ps)), f"admit: text_start {starts} - one per row, 0 .. P_r"
        limits = None
        if max_new_tokens is not None or self.limit_lens is not None:
            assert self.limit_lens is not None, "admit: max_new_tokens needs the stop rule's limits - set_stopping first"
            new = [cap] * R if max_new_tokens is None else per_row(max_new_tokens)
            assert len(new) == R and min(new) >= 0, f"admit: max_new_tokens is one non-negative int, or one per row ({R})"
            limits = [cap if max_new_tokens is None else s + v for s, v in zip(starts, new)]
            assert max(limits) <= cap, f"admit: text_start + max_new_tokens {limits} is beyond the history's capacity {cap}"
        assert start_states is None or self._fsm is not None, "admit: start_states are the states of a constraint - set_constraint first"
        st = None
        if self._fsm is not None:
            st = [0] * R if start_states is None else per_row(start_states)
            assert len(st) == R, f"admit: start_states is one int, or one per row ({R})"
        maxP = max(Ps)
        assert chunk is None or int(chunk) >= 1, f"admit: chunk={chunk} (None, or at least one token per sequence and pass)"
        chunk = maxP if chunk is None else min(int(chunk), maxP)
        i32 = dict(dtype=torch.int32, device=dev)
        all_rows, rows = rows, rows[:R]                                     # leaders, then followers
        rows_t = torch.tensor(rows, dtype=torch.int64, device=dev)
        all_t, lead_t = rows_t, None
        if len(lead) > R:
            all_t, lead_t = torch.tensor(all_rows, dtype=torch.int64, device=dev), torch.tensor(lead, dtype=torch.int64, device=dev)
        every = lambda v: [v[i] for i in lead]                              # noqa: E731
        P_t = torch.tensor(Ps, **i32)
        # ---- the rows' state that the pass does not compute: text, where it begins, its limit; live again
        text = torch.zeros((R, cap), dtype=torch.int32)
        for i, p in enumerate(pl):
            text[i, :Ps[i]] = p.to(torch.int32)
        text_d = text.to(dev)                                               # the one upload of the prompts
        self.history[all_t] = text_d if lead_t is None else torch.index_select(text_d, 0, lead_t)
        self.prompt_lens[all_t] = torch.tensor(every(starts), **i32)
        self._text_starts = self._row_starts()
        for r, s in zip(all_rows, every(starts)):
            self._text_starts[r] = s
        if limits is not None:
            self.limit_lens[all_t] = torch.tensor(every(limits), **i32)
        if self.finished is not None:
            self.finished[all_t] = 0
        if st is not None:
            self.fsm_state[all_t] = torch.tensor(every(st), **i32)
        if self._lora and lead_t is not None:                                    # a follower's prompt pages are its leader's: so is its adapter
            self.lora_ids[all_t] = torch.index_select(self.lora_ids, 0, rows_t)[lead_t]
        # ---- pages: the rows give back what they own and take their prompts' (two launches).  Under a prefix cache the whole pages of
        # a prompt's beginning that are cached - at most those below its last token, which is always recomputed: the head needs its
        # hidden row - are mapped into the row by a hold between the two, and the reserve grows the row behind them.  What a request
        # of THIS admit computes is entered at the end: two requests with the same new prefix in one admit do not share
        cached = [[] for _ in rows]
        if self.pager is not None:
            extra = torch.zeros((B,), **i32)
            extra[rows_t] = P_t
            if self.prefix is not None:
                cached = [self.prefix.match(p.tolist(), limit=P - 1) for p, P in zip(pl, Ps)]
            self.release_rows(all_rows)
            if any(cached):
                self.pager.hold({r: ids for r, ids in zip(rows, cached) if ids})
            self.pager.reserve(self._all_rows, 0, extra_rows=extra, finished=self.finished if self.stopping is not None else None)
        # ---- the prompts, in passes of `chunk` tokens per sequence, over the rows' table rows (read AFTER the reserve filled them)
        lora_ids = torch.index_select(self.lora_ids, 0, rows_t) if self._lora else None
        if not any(cached):
            last = self._prompt_pass(text_d[:, :maxP].to(torch.int64), Ps, chunk, self._prompt_buffers(R * chunk), 0,
                                     self._append_over([t[rows_t] for t in self.tables]), lora_ids)
        else:                                                               # only what is not cached: tokens[c_r:] at past c_r + c0
            cs = [64 * len(ids) for ids in cached]
            rest = torch.zeros((R, maxP), dtype=torch.int64)
            for i, p in enumerate(pl):
                rest[i, :Ps[i] - cs[i]] = p[cs[i]:]
            lens = [P - c for P, c in zip(Ps, cs)]
            chunk = min(chunk, max(lens))
            last = self._prompt_pass(rest.to(dev), lens, chunk, self._prompt_buffers(R * chunk), cs,
                                     self._append_over([t[rows_t] for t in self.tables], max(cs)), lora_ids)
        if self.prefix is not None:                                         # one read-back: where the rows' pages are
            page_ids = torch.index_select(self.pager.page_ids, 0, rows_t).cpu().tolist()
            new = []
            for r, p, P, ids, row_ids in zip(rows, pl, Ps, cached, page_ids):
                fresh = self.prefix.insert(p.tolist(), row_ids[:P // 64]) if min(row_ids[:P // 64], default=0) >= 0 else []   # (a starved row: nothing)
                self._row_cached[r] = ids + fresh
                new += fresh
            if new:
                self.pager.hold({}, hold_ids=new)
        # ---- the followers: the prompt's whole pages shared, the partly filled one copied - one launch pair over texts of P_r + 1
        if lead_t is not None:
            told = torch.ones((B,), dtype=torch.int32)
            told[rows] = torch.tensor(Ps, dtype=torch.int32) + 1
            self._fork_pages([(r, rows[i]) for r, i in zip(all_rows[R:], lead[R:])], told.to(dev))
            last, P_t = torch.index_select(last, 0, lead_t), P_t[lead_t]
        # ---- the head and the tail over the admitted rows, then what they leave to the text
        self._prompt_head(last, P_t, all_t)
        if self.beams is not None and self.pager is not None:               # a row that was refused pages holds no text: no hypothesis
            self.beam_score.masked_fill_(torch.zeros((B,), dtype=torch.bool, device=dev).index_fill_(0, all_t, True) &
                                         (self.pager.starved != 0), float("-inf"))
        self.history[all_t, P_t.to(torch.int64)] = torch.index_select(self.tokens, 0, all_t).to(torch.int32)
        self._len_bound = max(self._len_bound, maxP + 1)
        if self.stopping is not None:                                       # the root check of set_stopping: a first token that is a
            self._stop_k.zero_()                                            # stop, or a row at its limit; every other row's current
            self._stop_update(self.tokens, accept_lens=self._stop_k, check_root=True)   # token was looked at when it was emitted

    def serve(self, requests, stop=(), parents=None, sampled=False, poll_every=8, chunk=None):
        """Serve a stream of requests through the fixed batch: `requests` is a list of (prompt_tokens, max_new_tokens), first come first
        served - or (prompt_tokens, max_new_tokens, n) for n samples of one prompt (needs a counted pool: share_pages=True or
        prefix_cache=True): the group is admitted in one admit(copy_rows=) once n rows are free, the samples share the prompt's whole
        pages, each is from then on a request of its own, and the result gains samples = [dict(tokens, reason, preempted_at)] * n
        (the top-level entries are sample 0's), stats gains forked.  Starts from the empty batch (enable_drafting(None), set_stopping(stop, 0): every row frozen), then loops:
          1. the rows that finished hand their texts over (a device copy of their history rows; the texts are read once, at the end),
          2. their pages are released,
          3. waiting requests are admitted into free rows, in order, while the pool's free count covers ceil((P + 1) / 64) pages each,
          4. the captured step graph - with `parents`, the captured speculate graph - is replayed `poll_every` times (generate()'s
             burst),
          5. (`finished`, `lengths`, the pool's `count` and `owned`) are read back in one copy.
        Every decision is a `serving.Scheduler`'s - which rows ended, what a row that ended with NO_PAGES is PREEMPTED to, what is placed
        where, the page accounting, `stats`, the end; this loop performs them.  A preempted request's prompt is recomputed; reading its
        text is one more read-back for the bursts that preempt.  A resumed text need not be bit-identical to an un-preempted one:
        prompt and decode attention round differently, sampler keys follow the row, and log entries from before a preemption are lost.
        Under a prefix cache a request is charged only the pages its prompt cannot map, cached pages no row holds are evicted (one
        launch) when the free ones do not cover an admission, and a preempted row's whole pages are entered into the cache before it
        lets go, so the resumed request maps them again; stats gains hit_tokens, evicted, inserted_pages, every result hit_tokens.
        Raises before anything runs for a request that can never fit max_len (P + max_new > max_len) or the pool
        (ceil((P + max_new - 1 + n) / 64) > N, n the round's tokens: 1, or the tree's nodes).
        -> (per request, in order, dict(tokens: the generated text, reason: 1 a stop / 2 the length, preempted_at: the generated
        tokens it held at each preemption), stats dict(rounds, read_backs, admitted, preempted, peak_pages: the most pages in use at a
        read-back - the static batch * mb without a pool))."""
        self._single_gpu("serve")
        self._no_beams("serve", "its scheduler admits and releases single rows, a beam group lives and ends as a whole")
        assert poll_every >= 1
        B, dev = self.B, self.dev
        adv = 1 if parents is None else len(self._tree_arg(parents, "serve", drafting=False))
        sched = servingmod.Scheduler(requests, B, self.max_len, stoppingmod.NO_PAGES, pool_pages=None if self.pager is None else self.pager.N,
                                     advance=adv, static_pages=B * self.mb, prefix=self.prefix)
        assert len(sched.reqs) == len(sched.groups) or self.pager.refs is not None, \
            "serve: the samples of a request with n > 1 share pages of a counted page pool - DecodeEngine(page_pool=N, share_pages=True) " \
            "(or prefix_cache=True)"
        self.set_stopping(None)
        self.enable_drafting(None, *(self._draft_params or ()))
        self.set_stopping(stop, 0)
        advance, run = self._round_graph("serve", parents, sampled)
        done = torch.zeros((max(len(sched.reqs), 1), self.max_len), dtype=torch.int32, device=dev)   # the finished texts, read once at the end
        while True:
            # 1., 2. harvest and release
            ended, starved = sched.ended()
            texts, kept = [], []
            if starved:
                starved_t = torch.tensor(starved, dtype=torch.int64, device=dev)
                texts = self.history[starved_t]
                if self.prefix is not None:                                 # the rows' pages join the one read-back of their texts
                    texts = torch.cat((texts, self.pager.page_ids[starved_t]), dim=1)
                texts = texts.cpu().tolist()
                if self.prefix is not None:
                    # a preempted row's text stays cached: its slots < lengths - 1 are valid, so the whole pages of text[:L - 1] are
                    # entered before the row lets go, and the resumed request maps them again unless they were evicted meanwhile
                    for b, row in zip(starved, texts):
                        text, ids = row[:self.max_len], row[self.max_len:]
                        n = (sched.lens[b] - 1) // 64
                        fresh = self.prefix.insert(text[:sched.lens[b] - 1], ids[:n]) if min(ids[:n], default=0) >= 0 else []
                        self._row_cached[b] = list(self._row_cached.get(b, ())) + fresh
                        kept += fresh
                    texts = [row[:self.max_len] for row in texts]
                    sched.stats["inserted_pages"] += len(kept)
            if kept:
                self.pager.hold({}, hold_ids=kept)                          # (the cache's holds, before the rows let go)
            for b, i in sched.retire(texts, {b: len(self._row_cached.get(b, ())) for b in ended} if self.prefix is not None else None):
                done[i].copy_(self.history[b])
            if ended:
                # a harvested row goes back to what enable_drafting(None) left: a one-token text at its limit, frozen, owning nothing -
                # the bound of the lengths then follows the running texts alone
                ended_t = torch.tensor(ended, dtype=torch.int64, device=dev)
                for t, v in ((self.lengths, 1), (self.prompt_lens, 0), (self.limit_lens, 0), (self.finished, stoppingmod.LENGTH)):
                    t[ended_t] = v
                self.history[ended_t, 0] = self.tokens[ended_t].to(torch.int32)
                for b in ended:
                    self._text_starts[b] = 0
                if self.pager is not None:
                    self.release_rows(ended)
            # 3. admit what the scheduler placed, behind the eviction it asks for (one launch)
            rows, batch, *evict = sched.place()
            if evict and evict[0][0]:
                self.evict_prefixes(*evict[0])
            if rows:
                before = len(self.prefix) if self.prefix is not None else 0
                self.admit(rows, [q["prompt"] for q in batch], max_new_tokens=[q["max_new"] for q in batch],
                           text_start=[q["start"] for q in batch], chunk=chunk,
                           copy_rows=[sched.copy_rows.get(b, []) for b in rows] if sched.copy_rows else None)
                if self.prefix is not None:
                    sched.stats["inserted_pages"] += len(self.prefix) - before
            if sched.idle():
                break
            # 4., 5. a burst, and the one read-back
            burst = self._burst(run, advance, poll_every)
            assert burst >= 1, "serve: a round does not fit the page tables"
            parts = [self.finished, self.lengths] + ([] if self.pager is None else [self.pager.count, self.pager.owned])
            state = torch.cat(parts).cpu().tolist()
            sched.observe(burst, state[:B], state[B:2 * B], *(() if self.pager is None else (state[2 * B], state[2 * B + 1:])))
            self._len_bound = max(sched.lens)
        return sched.output(done.cpu().tolist())

    def _record_step(self, emitted=None):
        """history[b, lengths[b] - 1] = tokens[b], after step() advanced the lengths: history_append with a path of the root alone at
        past = lengths - 2 (its bonus token lands at past + 1).  A sequence that has outgrown `history` records nothing.  `emitted`:
        the k of set_stopping's rule (int32 [B], 0 / 1) in place of the constant ones - a sequence that emitted nothing records nothing."""
        nodes, idx, ones, past = self._step_record
        torch.sub(self.lengths, 2, out=past)
        draftingmod.history_append(self.history, past, nodes, idx, ones if emitted is None else emitted, self.tokens)

    def _tree_arg(self, parents, what, drafting=True):
        """`parents` of the entry `what` as a list, checked: a tree, on a single GPU, `drafting`: with a history to draft from."""
        from . import append as appendmod
        par = [int(p) for p in (parents.tolist() if hasattr(parents, "tolist") else parents)]
        self._single_gpu(what)
        self._no_beams(what, "beams under speculation are out of scope: a verification keeps one path per row")
        assert 1 <= len(par) <= appendmod.MAX_TREE and par[0] == -1 and all(0 <= p < i for i, p in enumerate(par) if i), \
            f"{what}: parents[0] = -1 (the root), every other node hangs off an earlier one; at most 64 nodes"
        assert not drafting or self.history is not None, f"{what}: enable_drafting first"
        return par

    def draft_tree(self, parents, out=None):
        """One n-gram draft tree per sequence from `history` (drafting.ngram_draft_tree with the parameters of enable_drafting) ->
        int64 [B, n] on the device; column 0 is the root, the current `tokens`.  Nothing leaves the device."""
        par = self._tree_arg(parents, "draft_tree")
        max_ngram, min_match, pad = self._draft_params
        return draftingmod.ngram_draft_tree(self.history, self.lengths, self._tree_constants(par)["tree"], max_ngram, min_match, pad, out=out)

    def speculate(self, parents, sampled=False):
        """One round of speculative decoding with nothing crossing to the host: draft_tree -> verify_tree(device_walk=True) ->
        drafting.history_append.  `tokens`, `lengths`, the cache and `history` end where accept_lens[b] decode steps would have left
        them.  -> the triple of verify_tree.  `sampled=True`: verify_tree(sampled=True), after set_sampling."""
        par = self._tree_arg(parents, "speculate")
        self._sampled_entry("speculate", sampled)
        return self._speculate(None, par, sampled=sampled)

    def _speculate(self, draft, par, max_past=None, out=None, sampled=False):
        """speculate() behind its argument checks.  `draft`: the [B, n] buffer the drafter fills (None: a fresh one); `max_past`, `out`:
        as for _verify_tree_device."""
        self._reserve(len(par))
        draft = self.draft_tree(par, out=draft)
        past = self.lengths - 1                                             # before the verification advances the lengths
        res = self._verify_tree_device(draft, par, max_past=max_past, out=out, sampled=sampled, reserved=True)
        draftingmod.history_append(self.history, past, draft, res[0], res[1], self.tokens)
        return res

    def capture_speculate(self, parents, max_past=None, sampled=False):
        """Capture one speculate() round of the tree `parents` in ONE hipGraph, the way capture_verify captures a verification
        (`_capture`: a warm-up round first), on one stream over persistent draft and output buffers.  run_speculate() replays it.
        `max_past`: the hint the split plan is frozen with (default: the engine's capacity, prompt_len + max_new); results never depend
        on it.  The warm-up is a real round: it advances `tokens`, `lengths`, the cache and `history` like any other.  `sampled=True`
        captures speculate(sampled=True) (after set_sampling).  Single GPU, with the lm_head, after enable_drafting."""
        par = self._tree_arg(parents, "capture_speculate")
        self._speculate_capture = self._capture_round("capture_speculate", par, self._speculate, max_past, sampled)
        self.speculate_graph = self._speculate_capture.graph
        return self.speculate_graph

    def run_speculate(self):
        """Replay the round capture_speculate captured: no argument, nothing copied from the host -> the persistent (accept_idx,
        accept_lens, argmax) tensors of the capture (overwritten by the next replay)."""
        assert self.speculate_graph is not None, "run_speculate: capture_speculate first"
        cap = self._speculate_capture
        self._fits("run_speculate", cap.n)
        self.speculate_graph.replay()
        self._len_bound += cap.n
        return cap.result

    # ---- one decode step (llama_w4a8_unpad.py:330-361 per layer) --------------------------------------------
    def _segments(self):
        """The step as a generator: yields the row-parallel partial output wherever tensor parallelism needs its sum
        all-reduce (2 per layer), so that the caller decides how the collective is issued (eagerly between hipGraph
        pieces, inside one graph, or not at all at world size 1)."""
        self._reserve(1)
        if self.with_lm_head:
            torch.index_select(self.embed, 0, self.tokens, out=self.hidden)
        bufs = dict(qa=self.q_act, qo=self.q_attn, q_mlp=self.q_mlp, q_scale=self.q_scale, q_sum=self.q_sum, qkv=self.qkv_buf,
                    proj=self.proj_out, proj_res=self.proj_res, gate_up=self.gate_up_buf, mlp_act=self.mlp_act)
        if self.moe is not None:
            bufs.update(normed=self.moe_normed, moe=self.moe_bufs)
        yield from self._layer_stack(self.hidden, bufs, self._step_attention, self.planes)
        layernorm_ops.rms_norm(self.final, self.hidden, self.norm_w, self.cfg["eps"])
        logits = None                                                # (the features of the tail need the un-cut head: _single_gpu)
        if self.with_lm_head and self.vocab_parallel:
            yield self._head_local()                                 # candidates of the ranks meet in the sum all-reduce
            self._head_finish(self.head_cand_res)
        elif self.with_lm_head:                                      # (penalty context: history[b, :lengths[b]], the text so far)
            logits = self._head(self.final, self.tokens, self._step_keys if self.sampling is not None else None, choose=self.beams is None)
            if self.beams is not None:
                self._beam_round(logits)
        k = self._emit(logits, self.tokens)                          # set_stopping: k = 0 (a stop before the new token, or a frozen row) / 1
        self.lengths.add_(1 if k is None else k)
        if self.history is not None:                                 # enable_drafting: the new token joins the text (k = 0: it does not)
            self._record_step(k)

    def _step_attention(self, li, qkv):
        """single_query_attention of layer li on the step's qkv rows -> q_attn / q_scale / q_sum, quantised."""
        cfg, B = self.cfg, self.B
        q, k, v = qkv.split([self.H * 128, self.Hkv * 128, self.Hkv * 128], dim=-1)
        q, k, v = q.reshape(B, self.H, 128), k.reshape(B, self.Hkv, 128), v.reshape(B, self.Hkv, 128)
        if self.fuse_pairs:  # attention + invoke_quant(_fuse_sum) of its output in one call (bit-identical pair fusion)
            fusedmod.single_query_attention_quant(
                q, k, v, self.tables[li], self.lengths, self.q_attn, self.q_scale, 8192, 64, self.size_per_token, self.max_len, 128,
                self.rope_base, True, self.int4, True, quant_sum=self.q_sum if self.group_size == -1 else None)
        else:
            attn = fused_attention.single_query_attention(
                q, k, v, self.tables[li], self.lengths, None, 8192, 64, self.size_per_token, self.max_len, 128, self.rope_base, True,
                self.int4, True)
            self._quant(self.q_attn, attn.reshape(B, -1), self.q_sum, self.q_scale)

    def _head_local(self):
        """This rank's greedy candidate per sequence -> its slot of `head_cand` (the other slots zero)."""
        logits = torch.matmul(self.final, self.lm_head.t())          # [B, V/N]
        argmax_rows_(logits, self.head_idx)
        val = logits.gather(1, self.head_idx.unsqueeze(1)).squeeze(1)
        gi = self.head_idx + self.v0
        self.head_cand.zero_()
        row = self.head_cand[self.tp_rank]
        row[:, 0] = val
        row[:, 1] = (gi & 2047).to(torch.float16)
        row[:, 2] = (gi >> 11).to(torch.float16)
        return self.head_cand.view(-1)

    def _head_finish(self, gathered):
        """tokens = the first maximum over the ranks' candidates (ranks own ascending vocabulary ranges, torch.argmax
        returns the first maximal entry: the same tie rule as an argmax over the whole row)."""
        c = gathered.float()                                          # [N, B, 8]
        best = c[:, :, 0].argmax(dim=0)
        sel = c.gather(0, best.view(1, -1, 1).expand(1, c.size(1), 8)).squeeze(0)
        self.tokens.copy_((sel[:, 1] + sel[:, 2] * 2048.0).to(torch.int64))

    def _reduce(self, partial):
        if self.ar is not None:
            self.ar.all_reduce(partial.numel())       # a kernel on the current stream (capturable)
        else:
            tpmod.all_reduce_sum_(partial)

    def step(self):
        for partial in self._segments():
            self._reduce(partial)
        self._len_bound += 1

    def _warm_up(self, fn):
        """fn() once on a side stream, outside any capture (allocator, lazy initialisation, the split-KV workspace - whose first use
        must not fall inside a capture), joined and synchronised.  A real call: it advances the engine like any other."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()

    def _capture(self, fn, advance):
        """Warm fn up, then capture it in one hipGraph -> (the graph, what the captured call returned: tensors the replays overwrite).
        `advance`: what one call of fn adds to `_len_bound` - taken back for the captured call, which has not run: only replays advance
        the lengths.  Frozen into the graph: which launches exist (sampling or arg-max and its seed, penalties, the history record)
        and the planner hints; read at replay: every persistent device tensor, the parameters of set_sampling / set_penalties among
        them."""
        self._warm_up(fn)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = fn()
        self._len_bound -= advance
        return g, res

    def capture(self, piecewise=None):
        """Capture one step in hipGraph(s) (removes ~400 launches of host overhead per step).

        World size 1: one graph.  Tensor parallel (default `piecewise`): one graph per segment between the all-reduces,
        the collectives themselves are issued eagerly between the replays - nothing depends on the communication
        library supporting stream capture, and the host only issues ~2 calls per layer and rank.
        `piecewise=False` captures the collectives too (needs a capturable backend)."""
        if piecewise is None:
            piecewise = self.tp_world > 1 and self.ar is None   # the direct all-reduce is an ordinary kernel: one graph
        self.pieces = None
        if not piecewise:
            self._step_capture = self._captured(self._capture(self.step, 1), 1)
            self.graph = self._step_capture.graph
            return self.graph
        self._warm_up(self.step)
        pool = torch.cuda.graph_pool_handle()
        pieces, gen = [], self._segments()
        while True:
            g = torch.cuda.CUDAGraph()
            partial = None
            # thread-local error mode: the process group's watchdog thread may poll its events while a piece is captured
            with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                try:
                    partial = next(gen)
                except StopIteration:
                    pass
            pieces.append((g, partial))
            if partial is None:
                break
            self._reduce(partial)             # keeps the data flow of the capture pass identical to a real step
        self.pieces = pieces
        self.graph = self._step_capture = None
        return pieces

    def check(self):
        """Raise if a bounded in-launch wait gave up since the last call (the library's direct all-reduce waiting for a
        peer): the tensors of that step are undefined.  Synchronises the device - call it once per batch of steps, not
        per step.  Under a page pool also: raise if a reserve or release met a broken invariant, or - while the stop rule is off, when
        nothing else would tell - if a row was refused pages."""
        if self.pager is not None:
            self.pager.check(starved=self.stopping is None)
        if self.ar is not None and self.ar.error():
            raise RuntimeError("direct all-reduce: a wait for a peer rank timed out (ranks more than a few seconds apart, or "
                               "a peer died); the communicators' epochs no longer match - re-create them")
        bits = _device_status()                        # K-slice seam of the GEMMs / attention + quant hand-over
        if bits:
            raise RuntimeError(f"a bounded in-launch wait of libqserve_amd gave up (error bits {bits}: 1 = K-slice seam of a W4A8 "
                               "GEMM, 2 = attention + quant hand-over): the tensors of that step are undefined; call "
                               "qserve_amd._lib.lib.qs_device_reset() before the next step")

    def run(self):
        if self.pieces:
            for g, partial in self.pieces:
                g.replay()
                if partial is not None:
                    self._reduce(partial)
            self._len_bound += 1
        elif self.graph is not None:
            self.graph.replay()
            self._len_bound += 1
        else:
            self.step()
