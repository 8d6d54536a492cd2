#!/usr/bin/env python
"""bench.py — coarse-retrieval queries/sec over the ~11k-cell database (BASELINE.json metric).

One "step" = one pass of the hot path over one batch: Q=4,096 precomputed text embeddings searched against
the resident N=11,259 x 256 cell database (BASELINE.json configs[1]: "~11k cells, embed_dim=256, 1xMI355X,
frozen T5-large embeddings precomputed"), top-10 ids + float64 scores out. Inputs are resident in HBM when
the timed region starts. With --gpus N the DB is row-sharded over the ranks (one process per GPU), every rank
searches its shard, one RCCL all_gather of the per-shard top-k, merge on every rank (strong scaling: total
work fixed).

Prints ONE JSON line on rank 0 (contract in the task statement). A plain run does set-up, warmup, the timed steps and
(--dump-outputs DIR) writes the last timed step's results, nothing else. --full adds everything measured or checked
beside the headline, with the line carrying it: `roofline` (dominant kernel = the fused MFMA candidate scan; algorithmic
FLOPs = 2*Q*N*D per launch / its hipEvent-measured duration vs the dense MFMA peak of the dtype the scan multiplies in:
2.5 PF for the default f16 scan and for --mode 2 = split-bf16), `cpu_baseline` (the numpy oracle of
training/coarse.py:119-125 timed on this host), parity against the float64 C oracle, the side measurements.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from text2loc_amd import synth  # noqa: E402
from text2loc_amd.engine import Engine  # noqa: E402
from text2loc_amd.sharded import QueryShardedSearcher, ShardedSearcher, shard_bounds  # noqa: E402

N_CELLS, N_QUERIES, DIM, TOPK = 11259, 4096, 256, 10
_QS = None
_QUICK = False
F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (AMD's 5 PF figure is 2:1 sparse)


def cpu_baseline(db, qs, budget_s=12.0):
    """The oracle's restatement of the reference loop (float64 matvec + full argsort per query), numpy."""
    from oracle import t2l_oracle as O

    try:
        from threadpoolctl import threadpool_info
        threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        threads = os.cpu_count() or 1
    O.retrieve_topk(db, qs[:64], TOPK)  # warm-up
    done, t0 = 0, time.perf_counter()
    chunk = 512
    while time.perf_counter() - t0 < budget_s and done < 8 * len(qs):
        lo = done % len(qs)
        O.retrieve_topk(db, qs[lo:lo + chunk], TOPK)
        done += min(chunk, len(qs) - lo)
    dt = time.perf_counter() - t0
    return {"value": done / dt, "unit": "queries/s", "cores": int(threads), "kind": "port",
            "sample": f"{done} queries x N={len(db)} (float64 C@t + full argsort per query, numpy) in {dt:.1f}s"}


PMC_SOURCE = ("profiles/pmc_latest.json = the latest committed profiles/r*_pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, "
              "tools/profile.sh, separate runs as the MI355X guide prescribes; not measured in this run)")


_PMC_LIVE = {}


def measure_traffic_in_run(kernel_prefix="t2l::scanp_kernel"):
    """HBM-side bytes per launch of the dominant kernel measured IN THIS RUN: two extra `rocprofv3 --kernel-trace --pmc` passes
    (FETCH_SIZE, WRITE_SIZE: separate passes, as MI355X_MICROARCH.md prescribes; no trace domain beside the counters) of this
    very script in --quick form, as subprocesses outside the timed region. 2 x FETCH_SIZE + WRITE_SIZE, KiB -> bytes (the guide's
    gfx950 correction). Returns None (and the committed profile is used) when rocprofv3 is not on PATH or a pass fails."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    if os.environ.get("T2L_BENCH_CHILD") or not shutil.which("rocprofv3"):
        return None
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="t2l_pmc_")
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-secondary", "--no-pipelined",
               "--quick"]
        try:
            subprocess.run(cmd, env=dict(os.environ, T2L_BENCH_CHILD="1", TMPDIR="/tmp"), cwd="/tmp", timeout=240, capture_output=True, check=True)
            acc = []
            for f in glob.glob(os.path.join(d, "**", "p_counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r["Counter_Name"] == counter and r["Kernel_Name"].replace("void ", "").startswith(kernel_prefix):
                        acc.append(float(r["Counter_Value"]))
            if not acc:
                return None
            vals[counter] = (sum(acc) / len(acc), len(acc))
        except Exception:
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return {"hbm_bytes_per_launch": 2 * vals["FETCH_SIZE"][0] * 1024 + vals["WRITE_SIZE"][0] * 1024, "launches": vals["FETCH_SIZE"][1],
            "FETCH_SIZE_KiB": vals["FETCH_SIZE"][0], "WRITE_SIZE_KiB": vals["WRITE_SIZE"][0]}


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (profiles/pmc_latest.json, written
    by tools/pmc_summary.py: 2 x FETCH_SIZE + WRITE_SIZE, KiB -> bytes, gfx950 correction per MI355X_MICROARCH.md).
    None when no profile has been committed for this kernel name."""
    if kernel in _PMC_LIVE:
        return _PMC_LIVE[kernel]["hbm_bytes_per_launch"]
    try:
        d = json.load(open(os.path.join(REPO, "profiles", "pmc_latest.json")))
        return d[kernel]["hbm_bytes_per_launch"]
    except Exception:
        return None


def torch_train_step_ms(sd, cells64, anchor, steps=20):
    """Same-GPU stock-library comparator for the training step: the identical graph in PyTorch eager (rocBLAS/MIOpen
    kernels + autograd + torch.optim.Adam), dropout 0.1 — what the reference's train_epoch runs for the object branch."""
    import argparse
    import torch.nn.functional as F
    from text2loc_amd.cell_retrieval import CellRetrievalNetwork

    class _Txt(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        @property
        def device(self):
            return self.p.device

    args = argparse.Namespace(coarse_embed_dim=256, object_size=28, object_inter_module_num_heads=4,
                              object_inter_module_num_layers=2, class_embed=True, color_embed=True,
                              use_features=["class", "color", "position", "num"])
    m = CellRetrievalNetwork(synth.KNOWN_CLASS, synth.COLOR_NAMES, args, language_encoder=_Txt())
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    m = m.cuda().train()
    oe = m.object_encoder
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells64.items()}
    B = len(cells64["counts"])
    rows = torch.cat([torch.arange(min(int(c), 28)) + int(o) for c, o in zip(cells64["counts"], cells64["offsets"][:-1])]).cuda()
    slots = torch.cat([torch.arange(min(int(c), 28)) + 28 * i for i, c in enumerate(cells64["counts"])]).cuda()
    opt = torch.optim.Adam([p for n, p in m.named_parameters() if n.startswith(("object_encoder.", "obj_inter_module."))], lr=1e-3)

    def step():
        opt.zero_grad()
        emb = [F.normalize(oe.class_embedding(t["class_idx"].long()), dim=-1),
               F.normalize(oe.color_embedding(t["color_idx"].long()), dim=-1),
               F.normalize(oe.pos_encoder(t["center"]), dim=-1),
               F.normalize(oe.num_encoder((t["n_pts"].unsqueeze(-1) - 1826.6844940968194) / 2516.8905096993817), dim=-1)]
        e = F.normalize(oe.mlp_merge(torch.cat(emb, dim=-1)), dim=-1)
        x = torch.zeros(B * 28, 256, device="cuda").index_copy(0, slots, e[rows]).view(B, 28, 256).permute(1, 0, 2).contiguous()
        for layer in m.obj_inter_module:
            x = layer(x)
        pos = F.normalize(x.max(dim=0)[0])
        sim = anchor @ pos.t()
        num, den = torch.exp(torch.diag(sim) / 0.1), torch.exp(sim / 0.1)
        loss = torch.mean(-torch.log(num / den.sum(0)) - torch.log(num / den.sum(1)))
        loss.backward()
        opt.step()

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3



def full_train_step_measure(eng, p64, n_ramp, n_steps, B=64, n_hints=6, n_tok=16):
    import torch.nn.functional as F
    from text2loc_amd.cell_retrieval import LanguageEncoder

    enc = LanguageEncoder(256, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1,
                          llm_model=object(), tokenizer=None, input_dim=1024)
    enc.load_state_dict({k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(0).items()}, strict=False)
    enc = enc.cuda().train()
    hidden = 0.2 * torch.randn(B * n_hints, n_tok, 1024, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    opt = torch.optim.Adam(enc.parameters(), lr=1e-4)
    res = {}

    def step(i):
        on_engine = enc.use_engine_train_head
        eng.zero_grad()
        if on_engine:
            enc.engine_zero_grad()
        else:
            opt.zero_grad(set_to_none=False)
        anchor = F.normalize(enc.head(hidden, B))
        pos = eng.encode_cells_train(p64, dropout_p=0.1, seed=i)
        loss, ga, gp = eng.contrastive_loss(anchor.detach().contiguous(), pos, 0.1)
        eng.encode_cells_backward(gp)
        anchor.backward(ga)
        eng.adam_step(1e-3)
        if on_engine:
            enc.engine_adam_step(1e-4)  # t2l_text_adam_step: the head's 13.6 M parameters in one launch (what optim.Adam routes them to)
        else:
            opt.step()
        return loss

    # (the engine head's arithmetic: split-bf16 = its f32-class default, or bf16 operands; an f32-MFMA form measured SLOWER than the
    # PyTorch row below — 7.6 vs 5.6 ms — and was removed in round 5)
    for name, on, bf16 in (("engine_text_head_split_bf16", True, 2), ("engine_text_head_bf16", True, 1), ("pytorch_text_head_f32", False, 0)):
        enc.use_engine_train_head = on
        eng.set_option("train_bf16", bf16)
        if enc._th_train_engine is not None and on:
            enc._th_train_engine.set_option("text_train_bf16", bf16)
        eng.set_option("profile_events", 0)
        for i in range(max(3, n_ramp // 3)):
            step(i)
        if on:
            enc._th_train_engine.set_option("text_train_bf16", bf16)  # (the head's own engine context exists after the first step)
            for i in range(3):
                step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            last = step(100 + i)
        torch.cuda.synchronize()
        res[name] = {"ms_per_step_wall": (time.perf_counter() - t0) / n_steps * 1e3, "final_loss": float(last)}
        if on:
            te = enc._th_train_engine
            te.set_option("profile_events", 1)
            for nme in ("text_train_forward", "text_train_backward"):
                te.kernel_stats(nme)
            for i in range(5):
                step(500 + i)
            torch.cuda.synchronize()
            res[name]["text_head_forward_ms"] = te.kernel_stats("text_train_forward")[0]
            res[name]["text_head_backward_ms"] = te.kernel_stats("text_train_backward")[0]
            te.set_option("profile_events", 0)
    eng.set_option("train_bf16", 0)
    eng.set_option("profile_events", 1)
    tok = B * n_hints * n_tok
    flops = 3.0 * (2.0 * tok * (1024 * 3072 + 1024 * 1024 + 2 * 1024 * 4096) + 2.0 * B * n_hints * (1024 * 256 + 256 * (768 + 256 + 2048)))
    res["workload"] = f"B={B} descriptions x {n_hints} hints x {n_tok} tokens (T5-large width) + the B=64 object-branch step; head FLOPs fwd+bwd {flops / 1e9:.0f} G"
    res["text_head_algorithmic_gflop_fwd_bwd"] = flops / 1e9
    return res


def text_head_measure(eng, d_db_rows, n_desc, n_hints=6, n_tok=16):
    """a5 / f-4a: the head after T5 for one search step's worth of queries. `total_ms` = what LanguageEncoder.head costs now
    (t2l_text_head — split-f16 MFMA GEMMs — for the d=1024 layer + max + inter_mlp, PyTorch-ROCm for the 256-d half);
    the all-PyTorch path (round 2: 82 ms) and the plain-f16 option beside it; then the cold query path: T5 hidden states ->
    head -> t2l_search ids, on the device, one stream."""
    import torch.nn.functional as F
    from text2loc_amd.cell_retrieval import LanguageEncoder

    enc = LanguageEncoder(256, fixed_embedding=True, intra_module_num_layers=1, inter_module_num_layers=1,
                          llm_model=object(), tokenizer=None, input_dim=1024)
    sd = {k[len("language_encoder."):]: torch.from_numpy(v) for k, v in synth.make_language_head_weights(0).items()}
    enc.load_state_dict(sd, strict=False)
    enc = enc.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = 0.2 * torch.randn(n_desc * n_hints, n_tok, 1024, device="cuda", generator=g)

    def first_half_torch(h):  # language_encoder.py:127-136: intra layer(s) at d=1024 over tokens, max, Linear+BN -> [B*6,256]
        x = h.permute(1, 0, 2)
        for layer in enc.intra_module:
            x = layer(x)
        return enc.inter_mlp(x.permute(1, 0, 2).contiguous().max(dim=1)[0])

    def second_half(x):  # language_encoder.py:137-147 + F.normalize: the 256-d half
        x = x.view(n_desc, n_hints, -1).permute(1, 0, 2)
        for layer in enc.inter_module:
            x = x + layer(x)
        return F.normalize(x.max(dim=0)[0])

    def timed(fn, arg, reps=5):
        for _ in range(2):
            fn(arg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn(arg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, r

    heng = enc._head_engine(hidden.device)
    flops = 2.0 * hidden.shape[0] * n_tok * (1024 * 3072 + 1024 * 1024 + 2 * 1024 * 4096) + 2.0 * hidden.shape[0] * 1024 * 256
    with torch.no_grad():
        ms_t, mid_t = timed(first_half_torch, hidden, reps=3)
        ms_e, (mid_e, flag) = timed(lambda h: heng.text_head(h, check=False), hidden)
        overflow = bool(flag.item())
        heng.set_option("encoder_f16", 1)
        ms_f, (mid_f, _) = timed(lambda h: heng.text_head(h, check=False), hidden)
        heng.set_option("encoder_f16", 0)
        ms2, out_t2 = timed(second_half, mid_e)
        ms2e, (out_e2, flag2) = timed(lambda x: heng.text_inter(x, n_desc, check=False), mid_e.contiguous(), reps=20)
        e_inter = float((F.normalize(out_e2) - out_t2).abs().max())
        e1 = float((mid_e - mid_t).abs().max() / mid_t.abs().max())
        e2 = float((mid_f - mid_t).abs().max() / mid_t.abs().max())
        # cold query path: hidden states -> head (engine + 256-d half) -> normalise -> search against the resident DB
        def cold(h):
            q = F.normalize(enc.head(h, n_desc)).contiguous()
            return eng.search(q, TOPK)
        ms_cold, _ = timed(cold, hidden, reps=3)
        # the same query path behind the per-sentence T5 cache (text2loc_amd.text_cache): ~1,000 distinct template sentences held as
        # T5 hidden states in HBM (synthetic here: the image has no T5-large weights), descriptions arrive as the reference's
        # List[str]; (a) gather + t2l_text_head + t2l_text_inter, (b) eval-mode memo of the per-sentence vectors: gather + t2l_text_inter
        from text2loc_amd.text_cache import TextCache
        n_distinct = 1000
        cache = TextCache(None, None, hidden.device, max_tokens=n_tok, dim=1024)
        cache.hidden = 0.2 * torch.randn(n_distinct, n_tok, 1024, device="cuda", generator=g)
        cache.n_tok = np.full((n_distinct,), n_tok, dtype=np.int32)
        cache.index = {f"s{i}.": i for i in range(n_distinct)}
        pick = np.random.default_rng(0).integers(0, n_distinct, size=(n_desc, n_hints))
        descs = [" ".join(f"s{j}." for j in row) for row in pick]
        enc.text_cache = cache

        def cold_cached(_):
            q = F.normalize(enc(descs)).contiguous()
            return eng.search(q, TOPK)
        cached = {}
        for memo in (False, True):
            enc.memoise_sentence_vectors = memo
            ms_c, (ci, _cs) = timed(cold_cached, None, reps=5)
            cached["memoised_sentence_vectors" if memo else "gather_plus_head"] = {"ms": ms_c, "queries_per_s": n_desc / (ms_c * 1e-3)}
        enc.text_cache = None
        h_ref = cache.hidden.index_select(0, torch.from_numpy(pick.reshape(-1)).cuda())
        ri, _rs = eng.search(F.normalize(enc.head(h_ref, n_desc)).contiguous(), TOPK)
        cached["ids_equal_uncached_path"] = bool(torch.equal(ci, ri))
        cached["cache"] = cache.stats()
    return {"workload": f"{n_desc} descriptions x {n_hints} hints x {n_tok} tokens, d=1024 (T5-large width)",
            "d1024_layer_plus_linear_ms": ms_e, "d256_half_ms": ms2e, "total_ms": ms_e + ms2e,
            "d256_half": {"engine_t2l_text_inter_ms": ms2e, "pytorch_rocm_eager_ms": ms2, "max_abs_err_of_unit_embeddings_vs_torch": e_inter,
                          "overflow_flag": bool(flag2.item()),
                          "tflops_algorithmic": 2.0 * n_desc * n_hints * 256 * (768 + 256 + 2 * 1024) / ms2e / 1e9},
            "engine_split_f16": {"ms": ms_e, "tflops_algorithmic": flops / ms_e / 1e9, "tflops_executed_f16": 3 * flops / ms_e / 1e9,
                                 "frac_of_f16_peak_executed": 3 * flops / ms_e / 1e9 / BF16_MFMA_PEAK_TFLOPS,
                                 "max_rel_err_vs_torch_f32": e1, "overflow_flag": overflow},
            "engine_plain_f16_option": {"ms": ms_f, "tflops": flops / ms_f / 1e9, "max_rel_err_vs_torch_f32": e2},
            "pytorch_rocm_eager_f32": {"d1024_layer_plus_linear_ms": ms_t, "total_ms": ms_t + ms2},
            "d256_half_share": ms2e / (ms_e + ms2e),
            "cold_query_path": {"what": f"T5 hidden states of {n_desc} descriptions -> LanguageEncoder.head (t2l_text_head + t2l_text_inter) -> "
                                        f"normalise -> t2l_search top-{TOPK} over {d_db_rows} cells, one stream, on the device",
                                "ms": ms_cold, "queries_per_s": n_desc / (ms_cold * 1e-3),
                                "note": "T5 itself is not in this number (no T5-large weights in the image): 4,096 x 6 x 16 tokens of "
                                        "T5-large are ~260 TFLOP per step on top of it",
                                "behind_the_sentence_cache": cached}}


def clustered_measure(eng, packed_cells):
    from oracle import c_oracle

    res = {}
    rs = np.random.default_rng(5)
    enc_db = eng.encode_cells(packed_cells)
    base = synth.unit_rows(rs.standard_normal((1, DIM)))
    packed_db = synth.unit_rows(base + 1e-3 * rs.standard_normal((N_CELLS, DIM))).astype(np.float32)
    cases = {"encoder_output_untrained": enc_db.cpu().numpy(), "one_direction_1e-3": packed_db}
    e2 = Engine(eng.device)
    for name, dbc in cases.items():
        tgt = rs.integers(0, len(dbc), size=N_QUERIES)
        spread = float(np.linalg.norm(dbc - dbc.mean(0), axis=1).mean())
        q = synth.unit_rows(dbc[tgt].astype(np.float64) + 0.25 * spread * synth.unit_rows(rs.standard_normal((N_QUERIES, DIM)))).astype(np.float32)
        dq = torch.from_numpy(q).cuda()
        e2.set_option("search_auto", 1)
        e2.db_set(torch.from_numpy(np.ascontiguousarray(dbc)).cuda())
        for _ in range(14):  # the auto mode settles within a few calls of a loop that consumes each result (report cards are read
            e2.search(dq, TOPK)  # when a call is enqueued)
            torch.cuda.synchronize()
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < 0.04:  # (clock ramp: the synchronised calls left the GPU mostly idle)
            for _ in range(8):
                e2.search(dq, TOPK)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 16
        for _ in range(reps):
            gi, gs = e2.search(dq, TOPK)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        flagged, stage3 = e2.search_rescored(), e2.search_fallbacks()
        sel = np.arange(0, N_QUERIES, 8)
        ridx, _ = c_oracle.retrieve_topk(dbc, q[sel], TOPK)
        res[name] = {"ms_per_step": dt * 1e3, "queries_per_s": N_QUERIES / dt, "flagged_share": flagged / N_QUERIES,
                     "exact_scan_share": stage3 / N_QUERIES, "mean_distance_to_centroid": spread,
                     "ids_equal_float64_oracle_on_sample": bool(np.array_equal(gi.cpu().numpy().astype(np.int64)[sel], ridx)),
                     "sample": int(len(sel))}
    e2.close()
    return res


def secondary_measurements(eng):
    """Outside the timed region: the fused cell encoder on the full 11,259-cell DB (cells/s, f32 MFMA TFLOP/s at the
    algorithmic 60.33 MFLOP/cell + 0.67 MFLOP/object of SURVEY.md §8d) and the contrastive loss step (us)."""
    out = {}
    sd = synth.make_object_branch_weights(0)
    eng.load_weights(sd, class_embed=True, color_embed=True)
    cells = synth.make_cells(N_CELLS, seed=4)
    packed = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells.items() if k != "counts"}
    for _ in range(12):  # (≈40 ms of this very kernel: the chip's sustained clocks, as for the headline loop)
        eng.encode_cells(packed)
    eng.kernel_stats("encode_cells")
    for _ in range(16 if not _QUICK else 5):
        eng.encode_cells(packed)
    torch.cuda.synchronize()
    ms, n = eng.kernel_stats("encode_cells")
    kept = np.minimum(cells["counts"], 28).sum()
    flops = N_CELLS * 60.33e6 + kept * 0.67e6
    tf = flops / (ms * 1e-3) / 1e12
    # default kernel: split-f16 MFMAs (3 f16 MFMA products per f32 product) for 97 % of the FLOPs -> priced against the f16
    # peak; `executed` is what the matrix pipe runs. The all-f32-MFMA kernel (option encoder_f32) is timed beside it.
    out["encode_cells"] = {"cells": N_CELLS, "kernel_ms": ms, "cells_per_s": N_CELLS / (ms * 1e-3),
                           "arithmetic": "split-f16 MFMA (hi*hi + hi*lo + lo*hi, f32 accumulate); attention core f32 MFMA",
                           "tflops_algorithmic": tf, "peak_tflops": BF16_MFMA_PEAK_TFLOPS, "frac": tf / BF16_MFMA_PEAK_TFLOPS,
                           "tflops_executed": 3 * tf, "frac_executed": 3 * tf / BF16_MFMA_PEAK_TFLOPS, "launches_timed": n}
    eng.set_option("encoder_f32", 1)
    for _ in range(2):
        eng.encode_cells(packed)
    eng.kernel_stats("encode_cells")
    for _ in range(3):
        eng.encode_cells(packed)
    torch.cuda.synchronize()
    ms32, _ = eng.kernel_stats("encode_cells")
    eng.set_option("encoder_f32", 0)
    out["encode_cells"]["f32_mfma_kernel"] = {"kernel_ms": ms32, "frac_of_f32_peak": flops / (ms32 * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS}
    # option encoder_f16: one f16 product per operand pair (the north star's bar is 1e-3 on the embeddings; the default holds 2e-7)
    ref_emb = eng.encode_cells(packed).clone()
    eng.set_option("encoder_f16", 1)
    for _ in range(10):
        emb16 = eng.encode_cells(packed)
    eng.kernel_stats("encode_cells")
    for _ in range(5):
        emb16 = eng.encode_cells(packed)
    torch.cuda.synchronize()
    ms16, _ = eng.kernel_stats("encode_cells")
    eng.set_option("encoder_f16", 0)
    out["encode_cells"]["plain_f16_option"] = {"kernel_ms": ms16, "cells_per_s": N_CELLS / (ms16 * 1e-3),
                                               "max_abs_diff_vs_default_embeddings": float((emb16 - ref_emb).abs().max()),
                                               "frac_executed": tf / BF16_MFMA_PEAK_TFLOPS}
    # (ii) cold end-to-end = encode the N cells from packed features + build the DB + search Q queries;
    # and the same-GPU stock-library comparator for the search (rocBLAS f32 GEMM + torch.topk, f32 scores only)
    try:
        dq_all = torch.from_numpy(np.ascontiguousarray(_QS)).cuda()
        eng_c = Engine(eng.device)
        eng_c.load_weights(sd, class_embed=True, color_embed=True)
        for _ in range(2):
            eng_c.db_set(eng_c.encode_cells(packed))
            eng_c.search(dq_all, TOPK)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng_c.db_set(eng_c.encode_cells(packed))
            eng_c.search(dq_all, TOPK)
        torch.cuda.synchronize()
        cold = (time.perf_counter() - t0) / 3
        out["cold_end_to_end"] = {"workload": f"encode {N_CELLS} cells + db_set + search {N_QUERIES} queries, top-{TOPK}",
                                  "ms": cold * 1e3, "queries_per_s": N_QUERIES / cold}
        eng_c.set_option("encoder_f16", 1)  # the same with the encoder's plain-f16 option (embeddings within ~1e-4)
        for _ in range(3):
            eng_c.db_set(eng_c.encode_cells(packed))
            eng_c.search(dq_all, TOPK)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng_c.db_set(eng_c.encode_cells(packed))
            eng_c.search(dq_all, TOPK)
        torch.cuda.synchronize()
        out["cold_end_to_end"]["ms_with_encoder_f16"] = (time.perf_counter() - t0) / 3 * 1e3
        eng_c.close()
        d_db = eng.encode_cells(packed)
        for _ in range(5):
            torch.topk(dq_all @ d_db.t(), TOPK, dim=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            torch.topk(dq_all @ d_db.t(), TOPK, dim=1)
        torch.cuda.synchronize()
        tt = (time.perf_counter() - t0) / 50
        out["torch_mm_topk_same_gpu"] = {"workload": "torch f32 [Q,256]@[256,N] (rocBLAS) + torch.topk(10): f32 ranking, not the "
                                                     "reference's float64 ranking", "ms_per_step": tt * 1e3,
                                         "queries_per_s": N_QUERIES / tt}
    except Exception as e:
        out["cold_end_to_end"] = {"error": repr(e)}
    # a2+a4 CPU baseline: the numpy restatement of ObjectEncoder.forward + encode_objects (the oracle,
    # threaded BLAS = all host cores) on B=64-cell batches, beside the encoder kernel's cells/s above
    try:
        from oracle import t2l_oracle as O
        c64 = synth.make_cells(64, seed=4)
        O.encode_cells(c64, sd, True, True)
        t0, reps = time.perf_counter(), 0
        while time.perf_counter() - t0 < 6.0:
            O.encode_cells(c64, sd, True, True)
            reps += 1
        dt = (time.perf_counter() - t0) / reps
        out["encode_cells"]["cpu_baseline"] = {"cells_per_s": 64 / dt, "kind": "port", "cores": os.cpu_count(),
                                               "sample": f"{reps} x 64 cells, numpy float32 restatement of object_encoder.py:66-153 + "
                                                         f"cell_retrieval.py:65-110 (eval mode)"}
    except Exception as e:
        out["encode_cells"]["cpu_baseline"] = {"error": repr(e)}
    # a5 / f-4, decided by data: the text head after T5 (language_encoder.py:127-148) on PyTorch-ROCm for one search step's
    # worth of queries (4,096 descriptions x 6 hints, 16 tokens each, T5-large width 1024), split into the d=1024
    # intra-layer + max + Linear/BN and the 256-d half (inter_module + max + normalize)
    try:
        out["text_head"] = text_head_measure(eng, N_CELLS, 512 if _QUICK else N_QUERIES)
    except Exception as e:
        out["text_head"] = {"error": repr(e)}
    # the data cliff: tightly clustered databases (what an encoder over overlapping cells produces) instead of the
    # friendly unit Gaussians of the headline — queries/s, share of queries the f16 certificate flags, share that ends in the
    # exact float64 scan. (a) DB = this engine's own (untrained) encoder output over the 11,259 synthetic cells;
    # (b) DB = one direction + 1e-3 perturbations. Queries = DB rows + noise, so every query has near ties.
    try:
        out["search_clustered"] = clustered_measure(eng, packed)
    except Exception as e:
        out["search_clustered"] = {"error": repr(e)}
    # the same step across data distributions: >= 6 tightness points between the headline's unit-Gaussian rows and the
    # one-direction database, plus a database produced by a TRAINED encoder over overlapping cells (bench_distribution.py)
    try:
        import bench_distribution
        out["search_distribution"] = bench_distribution.measure(N_CELLS, N_QUERIES, TOPK, quick=_QUICK)
    except Exception as e:
        out["search_distribution"] = {"error": repr(e)}
    # latency of small query batches against the resident DB (the reference answers one query at a time)
    lat = {}
    eng.set_option("profile_events", 0)  # (an event pair costs ~6 us per kernel: not inside a latency measurement)
    for qn in (1, 64):
        dq = torch.from_numpy(np.ascontiguousarray(_QS[:qn])).cuda()
        o = (torch.empty((qn, TOPK), dtype=torch.int32, device="cuda"), torch.empty((qn, TOPK), dtype=torch.float64, device="cuda"))
        n_ramp, n_lat = (10, 20) if _QUICK else (2000, 1000)
        if not _QUICK:  # clock ramp with REAL load first: single-query searches leave the GPU idle between launches and do not raise
            big = torch.from_numpy(np.ascontiguousarray(_QS)).cuda()  # the clocks of a chip that idled through the host phases before
            for _ in range(1200):
                eng.search(big, TOPK)
        for _ in range(n_ramp):
            eng.search(dq, TOPK, out=o)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_lat):
            eng.search(dq, TOPK, out=o)
        torch.cuda.synchronize()
        lat[f"q{qn}_us_per_call"] = (time.perf_counter() - t0) / n_lat * 1e6  # back to back on the stream
        t0 = time.perf_counter()
        for _ in range(20 if _QUICK else 200):
            eng.search(dq, TOPK, out=o)
            torch.cuda.synchronize()
        lat[f"q{qn}_us_per_call_synchronized"] = (time.perf_counter() - t0) / (20 if _QUICK else 200) * 1e6  # host-visible round trip of one call
    # the same single-query searches issued from C (t2l_search_many: 1,000 independent searches per call): what a search costs the
    # DEVICE back to back, without the ~14 us a Python ctypes call costs the host
    for qn in (1, 4, 16, 64):
        nb = 50 if _QUICK else 1000
        dqm = torch.from_numpy(np.ascontiguousarray(np.tile(_QS[:qn][None], (nb, 1, 1)))).cuda()
        om = (torch.empty((nb, qn, TOPK), dtype=torch.int32, device="cuda"), torch.empty((nb, qn, TOPK), dtype=torch.float64, device="cuda"))
        for _ in range(2):
            eng.search_many(dqm, TOPK, out=om)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 2 if _QUICK else 5
        for _ in range(reps):
            eng.search_many(dqm, TOPK, out=om)
        torch.cuda.synchronize()
        lat[f"q{qn}_us_per_call_issued_from_c"] = (time.perf_counter() - t0) / (reps * nb) * 1e6
        one_i, _ = eng.search(dqm[0].contiguous(), TOPK)
        lat[f"q{qn}_search_many_equals_search"] = bool(torch.equal(om[0][nb - 1], one_i))
        if qn <= 16:  # A/B, same box: the batched two-launch path these batches took until round 5 (option search_small = 0)
            ids_small = om[0][nb - 1].clone()
            eng.set_option("search_small", 0)
            for _ in range(2):
                eng.search_many(dqm, TOPK, out=om)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.search_many(dqm, TOPK, out=om)
            torch.cuda.synchronize()
            lat[f"q{qn}_us_per_call_issued_from_c_two_launch_path"] = (time.perf_counter() - t0) / (reps * nb) * 1e6
            lat[f"q{qn}_ids_equal_two_launch_path"] = bool(torch.equal(om[0][nb - 1], ids_small))
            eng.set_option("search_small", 1)
    eng.set_option("profile_events", 1)
    try:  # the one-launch kernel by itself (HIP events) and what that is against SURVEY 8d's per-query bound: 4 N D bytes per group of <= 4 queries
        dq1 = torch.from_numpy(np.ascontiguousarray(_QS[:1])).cuda()
        eng.kernel_stats("search_small")
        for _ in range(50):
            eng.search(dq1, TOPK)
        torch.cuda.synchronize()
        k_ms, k_n = eng.kernel_stats("search_small")
        if k_n:
            lat["q1_kernel_us"] = k_ms * 1e3
            lat["q1_algorithmic_bytes"] = 4.0 * N_CELLS * DIM
            lat["q1_kernel_GBps"] = 4.0 * N_CELLS * DIM / (k_ms * 1e-3) / 1e9
            lat["q1_frac_of_8TBps"] = lat["q1_kernel_GBps"] / 8000.0
            lat["q1_from_c_GBps"] = 4.0 * N_CELLS * DIM / (lat["q1_us_per_call_issued_from_c"] * 1e-6) / 1e9
    except Exception as e:
        lat["q1_kernel_error"] = repr(e)
    out["search_latency"] = lat
    # HBM-streaming regime (SURVEY.md §8d config 2'): 32 queries against N = 2,097,152 rows (1 GiB of f16 DB plane,
    # 4x the Infinity Cache): algorithmic bytes = that plane once per launch (512 B per row)
    try:
        n_big = 1 << 21
        rs = np.random.default_rng(7)
        big = rs.standard_normal((n_big, DIM), dtype=np.float32)
        big /= np.linalg.norm(big, axis=1, keepdims=True)
        eng2 = Engine(eng.device)
        eng2.set_option("profile_events", 1)
        eng2.db_set(torch.from_numpy(big).cuda())
        dq = torch.from_numpy(np.ascontiguousarray(_QS[:32])).cuda()
        for _ in range(3):
            eng2.search(dq, TOPK)
        eng2.kernel_stats("search_scan")
        for _ in range(10):
            idx_b, _ = eng2.search(dq, TOPK)
        torch.cuda.synchronize()
        ms, n = eng2.kernel_stats("search_scan")
        bytes_alg = n_big * 512.0
        sel = [0, 13, 31]
        from oracle import c_oracle
        ridx, _ = c_oracle.retrieve_topk(big, _QS[sel], TOPK)
        out["hbm_stream"] = {"workload": "N=2097152 rows (f16 plane 1 GiB), Q=32 per launch, top-10, scanq_kernel<16>", "kernel_ms": ms,
                             "algorithmic_bytes_per_launch": bytes_alg, "achieved_GBps": bytes_alg / (ms * 1e-3) / 1e9,
                             "peak_GBps": 8000.0, "frac": bytes_alg / (ms * 1e-3) / 1e9 / 8000.0,
                             "traffic": pmc_traffic("t2l::scanq_kernel<16>"), "launches_timed": n,
                             "ids_equal_float64_oracle_on_sample": bool(np.array_equal(
                                 idx_b.cpu().numpy().astype(np.int64)[sel], ridx))}
        eng2.close()
        del big
    except Exception as e:  # the side measurement must never take the headline down
        out["hbm_stream"] = {"error": repr(e)}
    # a1: per-object reductions over raw points (HBM-bound: 24 B per point, one pass)
    try:
        rs = np.random.default_rng(11)
        n_pts = np.clip(np.round(rs.lognormal(6.98, 1.0, size=16000)), 25, 60000).astype(np.int64)
        poff = np.zeros(len(n_pts) + 1, dtype=np.int64)
        np.cumsum(n_pts, out=poff[1:])
        total = int(poff[-1])
        d_xyz = torch.rand((total, 3), device="cuda")
        d_rgb = torch.rand((total, 3), device="cuda")
        d_off = poff
        rows = np.arange(8, dtype=np.int32)
        for _ in range(2):
            eng.reduce_objects(d_xyz, d_rgb, d_off, synth.COLORS, rows)
        eng.kernel_stats("reduce_objects")
        for _ in range(5):
            eng.reduce_objects(d_xyz, d_rgb, d_off, synth.COLORS, rows)
        torch.cuda.synchronize()
        ms, n = eng.kernel_stats("reduce_objects")
        out["reduce_objects"] = {"objects": len(n_pts), "points": total, "kernel_ms": ms,
                                 "achieved_GBps": total * 24.0 / (ms * 1e-3) / 1e9, "peak_GBps": 8000.0,
                                 "frac": total * 24.0 / (ms * 1e-3) / 1e9 / 8000.0, "launches_timed": n}
        del d_xyz, d_rgb
    except Exception as e:
        out["reduce_objects"] = {"error": repr(e)}
    # a3: PointNet++ object backbone on raw 256-point objects (published feature mode): split-f16 MFMA edge MLPs,
    # algorithmic ~376 MFLOP per object ("<=370 MFLOP/object")
    try:
        n_pc = 512
        cells_p = synth.make_cells(n_pc, seed=13)
        n_obj = int(cells_p["offsets"][-1])
        pos_np, rgb_np = synth.make_sampled_points(cells_p, 13)
        sd_pn = dict(sd)
        sd_pn.update(synth.make_pointnet_weights(0))
        eng_p = Engine(eng.device)
        eng_p.set_option("profile_events", 1)
        eng_p.load_weights(sd_pn, class_embed=False, color_embed=False)
        d_pos, d_rgb = torch.from_numpy(pos_np).cuda(), torch.from_numpy(rgb_np).cuda()
        for _ in range(4):
            eng_p.pointnet_features(d_pos, d_rgb, cells_p["offsets"])
        eng_p.kernel_stats("pointnet")
        for _ in range(6):
            f2 = eng_p.pointnet_features(d_pos, d_rgb, cells_p["offsets"])
        torch.cuda.synchronize()
        ms, n = eng_p.kernel_stats("pointnet")
        # executed edge-MLP rows: (128+4)*32, (64+2)*32, (32+1)*32 per object, + global MLP + FC
        fl = 2.0 * (132 * 32 * (8 * 32 + 32 * 64) + 66 * 32 * (72 * 128 + 128 * 128) + 33 * 32 * (136 * 256 + 256 * 256)
                    + 32 * (264 * 512 + 512 * 1024) + 1024 * 512 + 512 * 256)
        # spot check outside the timed region: the first two cells (their objects only see each other) vs the restatement
        from oracle import t2l_oracle_pointnet as OP
        n2 = int(cells_p["offsets"][2])
        ref2 = OP.pointnet_features(pos_np[:n2], rgb_np[:n2], cells_p["offsets"][:3], sd_pn)
        pn_err = float(np.abs(f2[:n2].cpu().numpy() - ref2).max())
        out["pointnet"] = {"objects": n_obj, "cells": n_pc, "kernel_ms": ms, "objects_per_s": n_obj / (ms * 1e-3),
                           "max_abs_err_vs_restatement_on_sample": pn_err, "sample_objects": n2,
                           "arithmetic": "split-f16 MFMA (3 f16 products per f32 product) with a magnitude watch; flagged objects "
                                         "are recomputed by the f32-MFMA kernels",
                           "tflops_algorithmic": fl * n_obj / (ms * 1e-3) / 1e12, "peak_tflops": BF16_MFMA_PEAK_TFLOPS,
                           "frac": fl * n_obj / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                           "frac_executed": 3 * fl * n_obj / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, "launches_timed": n,
                           "parity": "self-consistent only (third-party reference arithmetic, unpinned)"}
        eng_p.set_option("encoder_f16", 1)  # one f16 product per operand pair
        for _ in range(6):
            f2h = eng_p.pointnet_features(d_pos, d_rgb, cells_p["offsets"])
        torch.cuda.synchronize()
        eng_p.kernel_stats("pointnet")
        for _ in range(5):
            f2h = eng_p.pointnet_features(d_pos, d_rgb, cells_p["offsets"])
        torch.cuda.synchronize()
        ms_h, _ = eng_p.kernel_stats("pointnet")
        out["pointnet"]["plain_f16_option"] = {"kernel_ms": ms_h, "objects_per_s": n_obj / (ms_h * 1e-3),
                                               "max_abs_diff_vs_default": float((f2h - f2).abs().max()),
                                               "max_abs_feature": float(f2.abs().max())}
        eng_p.close()
    except Exception as e:
        out["pointnet"] = {"error": repr(e)}
    # a9 + a3: the backbone in TRAINING mode at the published batch (64 cells): per-cell BatchNorm statistics, full backward
    try:
        eng_t = Engine(eng.device)
        cells_t = synth.make_cells(64, seed=1)
        pos_t, rgb_t = synth.make_sampled_points(cells_t, 1)
        sd_t = dict(synth.make_object_branch_weights(2))
        sd_t.update(synth.make_pointnet_weights(1))
        tens = {}
        for k, v in sd_t.items():
            if k.endswith("num_batches_tracked") or k.endswith("_embedding.weight") or "classifier" in k:
                continue
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
        eng_t.train_bind(tens, class_embed=False, color_embed=False)
        offs_t = np.asarray(cells_t["offsets"], dtype=np.int32)
        dpos_t, drgb_t = torch.from_numpy(pos_t).cuda(), torch.from_numpy(rgb_t).cuda()
        g_t = torch.randn(pos_t.shape[0], 256, device="cuda")
        res = {}
        for variant, bf in (("f32", 0), ("split_bf16_gemms", 2), ("bf16_gemms", 1)):
            eng_t.set_option("train_bf16", bf)
            fw, bw = [], []
            for it in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng_t.pointnet_features_train(dpos_t, drgb_t, offs_t)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng_t.pointnet_backward(g_t)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it:
                    fw.append(t1 - t0)
                    bw.append(t2 - t1)
            res[variant] = {"forward_ms": 1e3 * min(fw), "backward_ms": 1e3 * min(bw), "step_ms": 1e3 * (min(fw) + min(bw))}
        eng_t.set_option("train_bf16", 0)
        free_b, total_b = torch.cuda.mem_get_info()
        out["pointnet_train_b64"] = dict(res, cells=64, objects=int(pos_t.shape[0]),
                                         parity="self-consistent only (float64 restatement + central differences, tests/test_gpu_pointnet_train.py)",
                                         note="wall clock around t2l_pointnet_features_train / t2l_pointnet_backward (the forward includes its "
                                              "index phase's host round trip)")
        eng_t.close()
        del tens
    except Exception as e:
        out["pointnet_train_b64"] = {"error": repr(e)}
    # f-1: fine stage on the coarse result — descriptors of all 11,259 database cells once, then Q x top-10 (pose, cell) pairs
    try:
        sd_f = synth.make_fine_weights(0)
        eng_f = Engine(eng.device)
        eng_f.set_option("profile_events", 1)
        eng_f.fine_load_weights(sd_f, class_embed=True, color_embed=True)
        cells16 = synth.make_cells(N_CELLS, seed=17, min_obj=16, max_obj=16)
        p16 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells16.items() if k != "counts"}
        for _ in range(2):
            desc = eng_f.fine_encode_objects(p16)
        eng_f.kernel_stats("fine_objects")
        for _ in range(3):
            desc = eng_f.fine_encode_objects(p16)
        torch.cuda.synchronize()
        ms_obj, _ = eng_f.kernel_stats("fine_objects")
        rs = np.random.default_rng(3)
        hints = torch.from_numpy(rs.standard_normal((N_QUERIES, 6, 128)).astype(np.float32)).cuda()
        ci = torch.from_numpy(rs.integers(0, N_CELLS, size=N_QUERIES * TOPK).astype(np.int32)).cuda()
        hi = torch.arange(N_QUERIES, dtype=torch.int32, device="cuda").repeat_interleave(TOPK).contiguous()
        for _ in range(8):  # (the host-side set-up above let the clocks drop: 40 ms of this kernel bring them back, README "clock ramp")
            eng_f.fine_match(desc, hints, ci, hi)
        eng_f.kernel_stats("fine_match")
        for _ in range(10):
            eng_f.fine_match(desc, hints, ci, hi)
        torch.cuda.synchronize()
        ms_m, _ = eng_f.kernel_stats("fine_match")
        n_pairs = N_QUERIES * TOPK
        # BASELINE config 5 (coarse + fine): search the resident DB, feed the retrieved row ids straight into the match
        dq_all = torch.from_numpy(np.ascontiguousarray(_QS)).cuda()
        for _ in range(2):
            top_idx, _s = eng.search(dq_all, TOPK)
            eng_f.fine_match(desc, hints, top_idx.reshape(-1).contiguous(), hi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            top_idx, _s = eng.search(dq_all, TOPK)
            off = eng_f.fine_match(desc, hints, top_idx.reshape(-1).contiguous(), hi)
        torch.cuda.synchronize()
        pipe = (time.perf_counter() - t0) / 3
        from oracle import t2l_oracle_fine as OF
        sel = np.arange(0, n_pairs, n_pairs // 8)[:8]
        ci_h, hi_h = top_idx.reshape(-1).cpu().numpy()[sel], hi.cpu().numpy()[sel]
        ref_off = OF.cross_match(OF.fine_object_encodings(cells16, sd_f, True, True)[ci_h], hints.cpu().numpy()[hi_h], sd_f)
        fine_err = float(np.abs(off.cpu().numpy()[sel] - ref_off).max())
        out["fine_stage"] = {"max_abs_err_vs_oracle_on_sample": fine_err, "coarse_plus_fine_ms": pipe * 1e3, "coarse_plus_fine_queries_per_s": N_QUERIES / pipe,"workload": f"{N_CELLS} padded cells x 16 objects -> descriptors; {N_QUERIES} queries x top-{TOPK} = {n_pairs} pairs",
                             "objects_kernel_ms": ms_obj, "match_kernel_ms": ms_m, "pairs_per_s": n_pairs / (ms_m * 1e-3),
                             "queries_per_s": N_QUERIES / (ms_m * 1e-3), "tflops_match": 23.0e6 * n_pairs / (ms_m * 1e-3) / 1e12,
                             "arithmetic": "split-f16 MFMA (3 f16 products per f32 product) behind a row-norm guard, attention core f32 MFMA "
                                           "(2 pairs per workgroup, register-resident attention, 3 workgroups per CU)",
                             "peak_tflops": BF16_MFMA_PEAK_TFLOPS,
                             "frac": 23.0e6 * n_pairs / (ms_m * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                             "frac_executed": 3 * 23.0e6 * n_pairs / (ms_m * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS}
        # option encoder_f16 (one f16 product per operand pair) on the match kernel
        eng_f.set_option("encoder_f16", 1)
        for _ in range(10):
            off16 = eng_f.fine_match(desc, hints, top_idx.reshape(-1).contiguous(), hi)
        eng_f.kernel_stats("fine_match")
        for _ in range(5):
            off16 = eng_f.fine_match(desc, hints, top_idx.reshape(-1).contiguous(), hi)
        torch.cuda.synchronize()
        ms16, _ = eng_f.kernel_stats("fine_match")
        out["fine_stage"]["plain_f16_option"] = {"match_kernel_ms": ms16, "pairs_per_s": n_pairs / (ms16 * 1e-3),
                                                 "max_abs_offset_diff_vs_default": float((off16 - off).abs().max()),
                                                 "max_abs_err_vs_oracle_on_sample": float(np.abs(off16.cpu().numpy()[sel] - ref_off).max())}
        eng_f.close()
    except Exception as e:
        out["fine_stage"] = {"error": repr(e)}
    # the same search with FOUR batches' worth of queries per call (Q = 16,384): what the scan kernel reaches when a launch's fixed
    # costs (dispatch, the cold start behind the kernel boundary, the candidate write-back) are spread over four times the work.
    # A side line: the headline's step stays Q = 4,096 per call.
    try:
        rs = np.random.default_rng(17)
        q_big = torch.from_numpy(np.concatenate([_QS] + [synth.unit_rows(rs.standard_normal(_QS.shape).astype(np.float32)) for _ in range(3)])).cuda()
        Qb = int(q_big.shape[0])
        ob = (torch.empty((Qb, TOPK), dtype=torch.int32, device="cuda"), torch.empty((Qb, TOPK), dtype=torch.float64, device="cuda"))
        eng.set_option("profile_events", 0)
        n_ramp_b, n_b = (5, 10) if _QUICK else (400, 200)
        for _ in range(n_ramp_b):
            eng.search(q_big, TOPK, out=ob)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_b):
            eng.search(q_big, TOPK, out=ob)
        torch.cuda.synchronize()
        tb = (time.perf_counter() - t0) / n_b
        eng.set_option("profile_events", 4)
        eng.kernel_stats("search_scan")
        for _ in range(24):
            eng.search(q_big, TOPK, out=ob)
        torch.cuda.synchronize()
        kb = eng.kernel_stats("search_scan")[0]
        eng.set_option("profile_events", 1)
        first = eng.search(torch.from_numpy(np.ascontiguousarray(_QS)).cuda(), TOPK)
        same = bool(torch.equal(ob[0][:N_QUERIES], first[0])) and bool(torch.equal(ob[1][:N_QUERIES], first[1]))
        fl_b = 2.0 * Qb * N_CELLS * DIM
        out["search_q16k_per_call"] = {"queries_per_call": Qb, "ms_per_call": tb * 1e3, "queries_per_s": Qb / tb, "scan_kernel_ms": kb,
                                       "scan_tflops": fl_b / (kb * 1e-3) / 1e12 if kb else None,
                                       "scan_frac_of_f16_peak": fl_b / (kb * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS if kb else None,
                                       "first_4096_rows_equal_the_4096_query_call": same}
    except Exception as e:
        out["search_q16k_per_call"] = {"error": repr(e)}
    # SURVEY.md 8e, measured on ONE GPU: what every rank of an 8-GPU row-sharded step does apart from the collective itself —
    # scan + re-rank over ceil(N/8) rows for ALL queries, pack the {score, id} records, merge 8 gathered lists per query.
    # This is the per-rank floor of config 3's step (the all_gather of 8 x 655 KB over xGMI comes on top).
    try:
        P = 8
        eng_s = Engine(eng.device)
        n_shard = -(-N_CELLS // P)
        rs = np.random.default_rng(5)
        shard = torch.from_numpy(synth.unit_rows(rs.standard_normal((n_shard, DIM)).astype(np.float32))).cuda()
        eng_s.db_set(shard, row_offset=0)
        dq_all = torch.from_numpy(np.ascontiguousarray(_QS)).cuda()
        Qn = int(dq_all.shape[0])
        allb, idx_s, sc_s, bb, so = eng_s.result_block(Qn, TOPK, "cuda", parts=P)   # P exchange blocks {ids | scores}; the views alias block 0
        m_out = (torch.empty((Qn, TOPK), dtype=torch.int32, device="cuda"), torch.empty((Qn, TOPK), dtype=torch.float64, device="cuda"))
        eng_s.search(dq_all, TOPK, out=(idx_s, sc_s))
        # stand-in for the all_gather: rank r's block = the real result of ANOTHER random shard of the same size for the same
        # queries (independent rows, as the shards of a real database are: the merge's work depends on how many of the 8 x K candidates
        # reach the bound — K .. 2K for independent shards; scaled copies of one list would make nearly all 80 survive), ids shifted
        for r in range(1, P):
            shard_r = torch.from_numpy(synth.unit_rows(np.random.default_rng(50 + r).standard_normal((n_shard, DIM)).astype(np.float32))).cuda()
            eng_s.db_set(shard_r, row_offset=r * n_shard)
            i_r, s_r = eng_s.search(dq_all, TOPK)
            blk_i = allb[r, :Qn * TOPK * 4].view(torch.int32).view(Qn, TOPK)
            blk_s = allb[r, so:so + Qn * TOPK * 8].view(torch.float64).view(Qn, TOPK)
            blk_i.copy_(i_r)
            blk_s.copy_(s_r)
        eng_s.db_set(shard, row_offset=0)
        eng_s.search(dq_all, TOPK, out=(idx_s, sc_s))
        eng_s.set_option("profile_events", 0)

        allv = allb.view(-1)

        def shard_step():  # (no allocation, no torch op: the host must not be what is measured)
            eng_s.search(dq_all, TOPK, out=(idx_s, sc_s))   # this rank's block, written in place (block 0 of the gathered buffer)
            return eng_s.merge_gathered(allv, bb, so, P, Qn, TOPK, out=m_out)

        n_ramp_s, n_s = (10, 20) if _QUICK else (1500, 400)
        for _ in range(n_ramp_s):
            shard_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_s):
            mi, ms_ = shard_step()
        torch.cuda.synchronize()
        t_all = (time.perf_counter() - t0) / n_s

        def only(fn):
            for _ in range(50 if not _QUICK else 5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_s):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n_s * 1e3

        t_search = only(lambda: eng_s.search(dq_all, TOPK, out=(idx_s, sc_s)))
        t_merge = only(lambda: eng_s.merge_gathered(allv, bb, so, P, Qn, TOPK, out=m_out))
        eng_s.set_option("profile_events", 1)
        for _ in range(20):
            shard_step()
        torch.cuda.synchronize()
        k_scan, k_rr = eng_s.kernel_stats("search_scan")[0], eng_s.kernel_stats("search_rerank")[0]
        k_merge = eng_s.kernel_stats("merge")[0]
        eng_s.set_option("profile_events", 0)
        from text2loc_amd.sharded import merge_topk_host
        hi_, hs_ = [], []
        for r in range(P):
            hi_.append(allb[r, :Qn * TOPK * 4].view(torch.int32).view(Qn, TOPK)[:256].cpu().numpy())
            hs_.append(allb[r, so:so + Qn * TOPK * 8].view(torch.float64).view(Qn, TOPK)[:256].cpu().numpy())
        ref_i, ref_s = merge_topk_host(np.stack(hi_), np.stack(hs_), TOPK)
        ok = bool(np.array_equal(mi[:256].cpu().numpy().astype(np.int64), ref_i)) and bool(np.array_equal(ms_[:256].cpu().numpy(), ref_s))
        out["shard_step_model"] = {"what": f"per-rank work of an {P}-GPU row-sharded step on one GPU: t2l_search over {n_shard} rows for all "
                                           f"{Qn} queries (ids | scores written straight into its exchange block) + t2l_merge_gathered(P={P}): three launches; the all_gather itself is not in it",
                                   "us_per_step": t_all * 1e6, "search_us_back_to_back": t_search * 1e3, "merge_us_back_to_back": t_merge * 1e3,
                                   "scan_kernel_us": k_scan * 1e3, "rerank_kernel_us": k_rr * 1e3, "merge_kernel_us": k_merge * 1e3,
                                   "note": "the *_back_to_back numbers are wall clock per call through the Python binding (a call costs ~14 us on "
                                           "the host whatever it launches: the merge loop is host-bound); kernel_us = HIP events around the launches; "
                                           "blocks 1..7 are real results of seven other random shards",
                                   "queries_per_s_if_the_collective_were_free": Qn / t_all, "merge_equals_host_merge_on_256_queries": ok}
        eng_s.close()
    except Exception as e:
        out["shard_step_model"] = {"error": repr(e)}
    # a9 / SURVEY.md §8d config 4: one training step of the object branch at B=64 (train-mode forward with dropout 0.1 ->
    # contrastive loss -> backward -> Adam), text side supplied as a precomputed [64,256] batch
    try:
        cells64 = synth.make_cells(64, seed=9)
        tens = {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or ".color_encoder." in k or ".mlp_pointnet." in k or ".pointnet." in k:
                continue
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            tens[k] = (t, None if "running_" in k else torch.zeros_like(t))
        eng.train_bind(tens, class_embed=True, color_embed=True)
        p64 = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells64.items() if k != "counts"}
        anchor = torch.nn.functional.normalize(torch.randn(64, 256, device="cuda"))

        def train_step(i):
            eng.zero_grad()
            pos = eng.encode_cells_train(p64, dropout_p=0.1, seed=i)
            loss, _, gp = eng.contrastive_loss(anchor, pos, 0.1)
            eng.encode_cells_backward(gp)
            eng.adam_step(1e-3)
            return loss

        # wall clock without event pairs (each costs the stream ~6 us) and after a clock ramp; phase times from a second, bracketed loop
        eng.set_option("profile_events", 0)
        n_ramp_t = 3 if _QUICK else 150
        for i in range(n_ramp_t):
            train_step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_steps = 5 if _QUICK else 100
        for i in range(n_steps):
            last = train_step(1000 + i)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n_steps
        eng.set_option("profile_events", 1)
        for nme in ("train_forward", "train_backward", "adam_step", "contrastive_loss"):
            eng.kernel_stats(nme)
        for i in range(3 if _QUICK else 30):
            train_step(100 + i)
        torch.cuda.synchronize()
        kept64 = int(np.minimum(cells64["counts"], 28).sum())
        fl = 3.0 * (64 * 60.33e6 + kept64 * 0.67e6)  # forward + 2x for backward (dX and dW contractions)
        out["train_step_b64"] = {"workload": "B=64 cells, %d objects, dropout 0.1, ContrastiveLoss(0.1), Adam" % int(cells64["offsets"][-1]),
                                 "ms_per_step_wall": wall * 1e3,
                                 "forward_ms": eng.kernel_stats("train_forward")[0],
                                 "backward_ms": eng.kernel_stats("train_backward")[0],
                                 "adam_ms": eng.kernel_stats("adam_step")[0],
                                 "loss_ms": eng.kernel_stats("contrastive_loss")[0],
                                 "steps_per_s": 1.0 / wall, "algorithmic_tflops": fl / wall / 1e12,
                                 "final_loss": float(last)}
        # BASELINE config 4 names bf16: the same step with option train_bf16 (GEMM operands rounded to bf16, f32 accumulation,
        # everything else f32) — its time, and how far its embeddings / loss sit from the f32 step on identical inputs
        try:
            eng.set_option("train_bf16", 0)
            pos32 = eng.encode_cells_train(p64, dropout_p=0.0, seed=1).clone()
            l32 = float(eng.contrastive_loss(anchor, pos32, 0.1)[0])
            eng.set_option("train_bf16", 1)
            pos16 = eng.encode_cells_train(p64, dropout_p=0.0, seed=1).clone()
            l16 = float(eng.contrastive_loss(anchor, pos16, 0.1)[0])
            eng.set_option("profile_events", 0)
            for i in range(n_ramp_t):
                train_step(200 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_steps):
                train_step(2000 + i)
            torch.cuda.synchronize()
            eng.set_option("profile_events", 1)
            out["train_step_b64"]["bf16_variant"] = {"ms_per_step_wall": (time.perf_counter() - t0) / n_steps * 1e3,
                                                     "max_abs_embedding_diff_vs_f32": float((pos16 - pos32).abs().max()),
                                                     "loss_f32": l32, "loss_bf16": l16}
            # option train_bf16 = 2: split-bf16 (hi + lo operands, three MFMAs per 16-step): f32-class accuracy, bf16-class speed
            eng.set_option("train_bf16", 0)  # (the weights moved during the loop above: a fresh f32 reference on the current ones)
            pos32b = eng.encode_cells_train(p64, dropout_p=0.0, seed=1).clone()
            l32b = float(eng.contrastive_loss(anchor, pos32b, 0.1)[0])
            eng.set_option("train_bf16", 2)
            pos2 = eng.encode_cells_train(p64, dropout_p=0.0, seed=1).clone()
            l2 = float(eng.contrastive_loss(anchor, pos2, 0.1)[0])
            eng.set_option("profile_events", 0)
            for i in range(n_ramp_t):
                train_step(400 + i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_steps):
                train_step(3000 + i)
            torch.cuda.synchronize()
            eng.set_option("profile_events", 1)
            out["train_step_b64"]["split_bf16_variant"] = {"ms_per_step_wall": (time.perf_counter() - t0) / n_steps * 1e3,
                                                           "max_abs_embedding_diff_vs_f32": float((pos2 - pos32b).abs().max()),
                                                           "loss_f32": l32b, "loss_split_bf16": l2}
            eng.set_option("train_bf16", 0)
        except Exception as e:
            out["train_step_b64"]["bf16_variant"] = {"error": repr(e)}
        # the FULL published step (README.md:87-99 trains the object branch AND the head after the frozen T5): text leaf = T5 hidden
        # states [64 x 6 sentences, 16 tokens, 1024] (what the sentence cache serves), LanguageEncoder.head under train() on the
        # engine (t2l_text_head_train / _backward, torch.optim.Adam on its 16.8 M parameters) + the object-branch step above + the
        # fused contrastive loss; beside it the same step with the head on its PyTorch modules
        try:
            out["train_step_b64"]["full_step_with_text_head"] = full_train_step_measure(eng, p64, n_ramp_t, n_steps)
        except Exception as e:
            out["train_step_b64"]["full_step_with_text_head"] = {"error": repr(e)}
        try:
            out["train_step_b64"]["torch_eager_ms_per_step_same_gpu"] = torch_train_step_ms(sd, cells64, anchor)
        except Exception as e:
            out["train_step_b64"]["torch_eager_error"] = repr(e)
    except Exception as e:
        out["train_step_b64"] = {"error": repr(e)}
    rng = np.random.default_rng(0)
    a = torch.from_numpy(rng.standard_normal((64, 256)).astype(np.float32)).cuda()
    p = torch.from_numpy(rng.standard_normal((64, 256)).astype(np.float32)).cuda()
    for _ in range(3):
        eng.contrastive_loss(a, p, 0.1)
    eng.kernel_stats("contrastive_loss")
    for _ in range(20):
        eng.contrastive_loss(a, p, 0.1)
    torch.cuda.synchronize()
    ms, n = eng.kernel_stats("contrastive_loss")
    out["contrastive_loss_b64_fwd_bwd_us"] = ms * 1e3
    if not _QUICK:
        # throughput AT THE BOUNDARY (round-5 verdict item 1): run_coarse(model, dataloader, args) through the drop-in Python surface at
        # config-2 size, batch_size 1 and 64, embedding and published (PointNet++) feature mode — bench_e2e.py holds the full record
        try:
            import bench_e2e

            rec = bench_e2e.measure(quick=True)
            flat = {}
            for mode, r in bench_e2e.headline_brief(rec).items():
                flat[f"{mode}_bs1_wall_ms"] = r["bs1_wall_s"] * 1e3
                flat[f"{mode}_bs64_wall_ms"] = r["bs64_wall_s"] * 1e3
                flat[f"{mode}_first_call_ms"] = r["first_call_s"] * 1e3
                flat[f"{mode}_gpu_stages_ms"] = r["gpu_stages_s"] * 1e3
                flat[f"{mode}_wall_over_gpu_stages_frac"] = r["wall_over_gpu_stages"]
                flat[f"{mode}_one_call_per_item_bs1_full_size_ms"] = r["legacy_bs1_full_size_s"] * 1e3
                cpu = rec[mode].get("cpu_reference_style_encode") or {}
                if "extrapolated_db_side_s" in cpu:
                    flat[f"{mode}_cpu_reference_style_db_side_ms"] = cpu["extrapolated_db_side_s"] * 1e3
            flat["n_cells"], flat["n_poses"] = rec["n_cells"], rec["n_poses"]
            out["run_coarse_e2e"] = flat
            out["run_coarse_e2e_detail"] = {"record": rec}
        except Exception as e:
            out["run_coarse_e2e"] = {"error": repr(e)}
        # the default arithmetic, decided with data (verdict item 5): a model TRAINED on the synthetic dataset, its database built in
        # split-f16 (default) and in plain f16 (option encoder_f16), the same queries: id agreement and recall deltas (tools/arith_ab.py)
        try:
            import importlib.util

            spec = importlib.util.spec_from_file_location("arith_ab", os.path.join(REPO, "tools", "arith_ab.py"))
            ab = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(ab)
            r = ab.measure(published=False, epochs=6)
            d = r["all_f16_vs_exact"]
            out["arithmetic_ab"] = {"mode": "embed", "recall_top1_exact_frac": r["recall"]["exact"]["top1"], "recall_top1_plain_f16_frac": r["recall"]["all_f16"]["top1"],
                                    "recall_top5_exact_frac": r["recall"]["exact"]["top5"], "recall_top5_plain_f16_frac": r["recall"]["all_f16"]["top5"],
                                    "same_id_list_top1_frac": d["same_list_top1"], "same_id_list_top5_frac": d["same_list_top5"],
                                    "same_id_list_top10_frac": d["same_list_top10"], "max_abs_cell_embedding_diff": d["max_abs_cell_embedding_diff"],
                                    "exact_run_repeats_bit_for_bit": r["exact_run_repeats_bit_for_bit"],
                                    "decision": "split-f16 stays the default: plain f16 keeps every recall figure but reorders the top-10 id list of 1-4 % of the "
                                                "queries (north star: integer-exact ids)"}
            out["arithmetic_ab_detail"] = {"record": r}
        except Exception as e:
            out["arithmetic_ab"] = {"error": repr(e)}
    return out


def roofline(kname, peak, mult, flops, scan_ms, scan_n, span_ms, span_n, busy_ms, busy_n):
    """achieved = ALGORITHMIC flops (2*Q*N*D) of one scan launch / the scan kernel's average duration (HIP events on sampled
    launches of the timed region and of the same loop right behind it; rocprofv3 agrees, profiles/). `peak` is the dense MFMA
    peak of the dtype the pipe runs in (f16 and bf16 share the 2.5 PF rate). In --mode 2 every product is 3 bf16 MFMA
    products: `executed` / `frac_executed` give the matrix pipe's view."""
    achieved = flops / (scan_ms * 1e-3) / 1e12 if scan_ms and scan_ms > 0 else 0.0
    return {"bound": "mfma", "kernel": kname, "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "executed": achieved * mult, "frac_executed": achieved * mult / peak,
            "time_basis": "scan kernel average duration, HIP events on sampled launches of the timed region and of the 64 steps of the same loop behind it",
            "traffic": pmc_traffic("t2l::" + kname),
            "traffic_source": ("measured in this run: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) of `bench.py --quick` as subprocesses "
                               "outside the timed region, 2 x FETCH_SIZE + WRITE_SIZE" if ("t2l::" + kname) in _PMC_LIVE else PMC_SOURCE),
            "traffic_detail": _PMC_LIVE.get("t2l::" + kname),
            "kernel_ms": scan_ms, "launches_timed": scan_n,
            "kernel_ms_in_kernel_span": span_ms, "launches_timed_in_kernel_span": span_n,
            # sum of the launch's workgroup durations / grid (in-kernel stamps, every launch): the GPU time a launch used
            "kernel_ms_gpu_time": busy_ms, "launches_timed_gpu_time": busy_n,
            "flops_per_launch": flops,
            # what the matrix pipe sustains on dense RANDOM f16 operands (power-limited clocks): measured IN THIS RUN by
            # tools/pair_probe.hip (bare v_mfma_f32_32x32x16_f16 stream; text2loc_amd/mfma_ceiling_probe.bin, built by `make`) —
            # absent when the probe is (no constant stands in for it)
            **mfma_ceiling_fields(achieved * mult)}


_CEILING = {}


def measure_mfma_ceiling():
    """Runs the MFMA probe once (outside every timed region, ~1 s) and keeps its best bare-stream rate (K = 0 fillers, one or two waves
    per SIMD) and the rate of the scan's own mix (7 fillers per MFMA, two waves per SIMD); None when the binary is missing."""
    if _CEILING:
        return _CEILING
    exe = os.path.join(REPO, "text2loc_amd", "mfma_ceiling_probe.bin")
    if not os.path.exists(exe):
        return None
    try:
        txt = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    except Exception:
        return None
    import re

    rows = re.findall(r"-> ([0-9.]+) TFLOP/s; K=\s*(\d+) waves/SIMD=(\d)", txt)
    bare = [float(t) for t, k, w in rows if int(k) == 0]
    mix = [float(t) for t, k, w in rows if int(k) == 7 and int(w) == 2]
    if not bare:
        return None
    _CEILING.update({"tflops": max(bare), "scan_mix_tflops": mix[0] if mix else None, "probe_output": txt.strip().splitlines()})
    return _CEILING


def mfma_ceiling_fields(executed_tflops):
    c = _CEILING or None
    if not c:
        return {}
    return {"measured_random_data_mfma_ceiling_tflops": c["tflops"], "frac_of_measured_ceiling": executed_tflops / c["tflops"],
            "measured_scan_mix_ceiling_tflops": c.get("scan_mix_tflops"),
            "ceiling_source": "tools/pair_probe.hip run in this process's run (bare random-operand v_mfma_f32_32x32x16_f16 stream)",
            "ceiling_probe_output": c.get("probe_output")}


HEADLINE_MAX_BYTES = 4096


def _r(x, nd=6):
    """floats to `nd` significant digits (the line is read by a parser with a small buffer); everything else untouched"""
    if isinstance(x, float):
        return float(f"{x:.{nd}g}")
    return x


def side_figures(sec):
    """The side measurements' key kernel / wall times (ms) as ONE flat object of the headline line, so that they are parsed with it
    (the SECONDARY line beside it is not JSON on purpose). Missing measurements are simply absent."""
    def g(*path):
        x = sec
        for k in path:
            if not isinstance(x, dict) or k not in x:
                return None
            x = x[k]
        return _r(x, 4) if isinstance(x, (int, float)) and not isinstance(x, bool) else None
    pairs = {"encode_cells_11259": g("encode_cells", "kernel_ms"), "pointnet_10698_objects": g("pointnet", "kernel_ms"),
             "fine_match_40960_pairs": g("fine_stage", "match_kernel_ms"), "text_inter_4096": g("text_head", "d256_half_ms"),
             "train_step_b64_f32": g("train_step_b64", "ms_per_step_wall"), "train_step_b64_bf16": g("train_step_b64", "bf16_variant", "ms_per_step_wall"),
             "pointnet_train_b64_f32": g("pointnet_train_b64", "f32", "step_ms"), "pointnet_train_b64_bf16": g("pointnet_train_b64", "bf16_gemms", "step_ms"),
             "run_coarse_embed_bs1": g("run_coarse_e2e", "embed_bs1_wall_ms"), "run_coarse_published_bs1": g("run_coarse_e2e", "published_bs1_wall_ms"),
             "run_coarse_published_gpu_stages": g("run_coarse_e2e", "published_gpu_stages_ms"),
             "search_q1_us": g("search_latency", "q1_us_per_call"), "search_q64_us": g("search_latency", "q64_us_per_call")}
    return {k: v for k, v in pairs.items() if v is not None}


def format_headline(d):
    """The ONE stdout JSON line of the contract, < 4 KB whatever the run measured: the contract's keys, `roofline` and
    `cpu_baseline` ADJACENT, parity, ranks_seen and (N > 1) the other layout's rate — every list, note and side measurement of
    the full record `d` stays in the detail file. Pure function of `d` (tests/test_bench_line.py feeds it canned numbers)."""
    rl, cb, par, cfg = d.get("roofline") or {}, d.get("cpu_baseline"), d.get("parity") or {}, d.get("config") or {}
    line = {k: _r(d.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                      "scaling", "vs_baseline", "dtype", "data")}
    line["config"] = {k: cfg.get(k) for k in ("workload", "n_cells", "queries_per_step", "embed_dim", "top_k", "parallelism", "layout")
                      if cfg.get(k) is not None}
    if rl:  # (a plain run, without --full, measures the headline only: no roofline, no CPU baseline, no parity)
        line["roofline"] = {k: _r(rl.get(k)) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms",
                                                       "launches_timed", "flops_per_launch")}
    if rl.get("frac_of_measured_ceiling") is not None:  # `peak` is the nominal rate; dense random-data MFMAs are power-limited below it
        line["roofline"]["measured_random_data_mfma_ceiling"] = _r(rl.get("measured_random_data_mfma_ceiling_tflops"))
        line["roofline"]["frac_of_measured_ceiling"] = _r(rl.get("frac_of_measured_ceiling"))
    if cb is not None:
        line["cpu_baseline"] = {k: _r(cb.get(k)) for k in ("value", "unit", "cores", "kind", "sample")}
        line["cpu_baseline"]["sample"] = str(line["cpu_baseline"]["sample"])[:160]
        line["speedup_vs_cpu_baseline"] = _r(d.get("speedup_vs_cpu_baseline"))
    if par:
        line["parity"] = {"ids_equal": par.get("ids_equal_float64_oracle"), "pairs_checked": par.get("pairs_checked"),
                          "max_abs_score_err": _r(par.get("max_abs_score_err"))}
    line["ranks_seen"] = d.get("ranks_seen")
    km = d.get("kernels_ms") or {}
    if km:
        line["kernels_ms"] = {k: _r(v) for k, v in km.items()}
    st = d.get("steady_state")
    if st:
        line["steady_state"] = {k: _r(st.get(k)) for k in ("steps", "untimed_ramp_steps", "ms_per_step", "queries_per_s")}
    for key, keep in (("alt_query_sharded", ("queries_per_s", "ms_per_step", "ids_equal_row_sharded")),
                      ("weak_scaling_point", ("rows_total", "queries_per_s", "ms_per_step", "error")),
                      ("config5_coarse_plus_fine", ("queries_per_s", "ms_per_step", "error"))):
        if d.get(key):
            line[key] = {k: (_r(d[key][k]) if not isinstance(d[key][k], str) else d[key][k][:120]) for k in keep if k in d[key]}
    side = side_figures(d.get("secondary") or {})
    if side:
        line["side_ms"] = side
    if d.get("detail_file"):
        line["detail_file"] = d["detail_file"]
    txt = json.dumps(line)
    if len(txt) >= HEADLINE_MAX_BYTES:  # cannot happen with the fields above; if a caller passes absurd strings, shed the optional ones
        for key in ("side_ms", "config5_coarse_plus_fine", "weak_scaling_point", "steady_state", "kernels_ms", "detail_file"):
            line.pop(key, None)
        line["config"]["workload"] = str(line["config"].get("workload"))[:200]
        txt = json.dumps(line)
    assert len(txt) < HEADLINE_MAX_BYTES, len(txt)
    return txt


def format_secondary(sec, max_bytes=3500):
    """One short NON-JSON stdout line (prefix `SECONDARY `, so that a line-wise JSON parser skips it) printed just before the headline:
    the side measurements' key figures, for a reader who only has the tail of stdout. Scalars only, depth <= 2, largest groups dropped first."""
    brief = {}
    for name, grp in (sec or {}).items():
        if not isinstance(grp, dict):
            if isinstance(grp, (int, float, bool)):
                brief[name] = _r(grp, 4)
            continue
        g = {}
        for k, v in grp.items():
            if isinstance(v, bool) or isinstance(v, (int, float)):
                g[k] = _r(v, 4)
            elif isinstance(v, dict):
                for k2, v2 in v.items():
                    if isinstance(v2, (int, float)) and not isinstance(v2, bool) and ("ms" in k2 or "frac" in k2 or "per_s" in k2 or "us" in k2):
                        g[f"{k}.{k2}"] = _r(v2, 4)
        if g:
            brief[name] = g
    txt = json.dumps(brief, separators=(",", ":"))
    while len(txt) > max_bytes and brief:
        biggest = max(brief, key=lambda n: len(json.dumps(brief[n])))
        if isinstance(brief[biggest], dict) and len(brief[biggest]) > 4:  # keep the timing-like keys of the biggest group only
            keep = {k: v for k, v in brief[biggest].items() if any(t in k for t in ("ms", "frac", "per_s", "us"))}
            brief[biggest] = dict(list(keep.items())[:4])
        else:
            brief.pop(biggest)
        txt = json.dumps(brief, separators=(",", ":"))
    return "SECONDARY " + txt


def main():
    global N_CELLS, N_QUERIES
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="also measure and check everything beside the headline: roofline, "
                    "steady state, parity vs the float64 C oracle, pipelined and N > 1 side lines, side measurements, CPU baseline, "
                    "the full record in --detail-out (the --no-* and --quick options below apply to these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's results as DIR/ids.npy and DIR/scores.npy (float64 [Q, top_k])")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the encoder / loss side measurements")
    ap.add_argument("--cells", type=int, default=N_CELLS, help="dev: database rows (default = the BASELINE workload)")
    ap.add_argument("--queries", type=int, default=N_QUERIES, help="dev: queries per step")
    ap.add_argument("--mode", type=int, default=0, choices=[0, 2], help="search_mode: 0 = f16 scan (default), 2 = split-bf16 scan")
    ap.add_argument("--nsplit", type=int, default=0, help="override the scan kernel's DB split count (0 = auto)")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the pipelined side measurement (profiling runs: its "
                    "overlapping launches would enter the per-kernel averages)")
    ap.add_argument("--quick", action="store_true", help="profiling runs (rocprofv3 --pmc slows every launch ~100x and does not "
                    "survive tens of thousands of them): no clock-ramp steps, short side loops, no pipelined measurement")
    ap.add_argument("--detail-out", default=os.path.join(REPO, "gpurun_out", "bench_detail.json"),
                    help="where the full record (side measurements, distribution lists, notes) goes; the stdout line stays < 4 KB")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher — N ranks of this same script, one per GPU, over RCCL
        # (exactly what `python -m torch.distributed.run --nproc-per-node N bench.py ...` does); rank 0 prints the JSON line
        import socket
        import subprocess
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.run(cmd, env=env).returncode)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    dev = local % max(ndev, 1)  # one process per GPU; the modulo only matters for the 1-GPU dry run of the N>1 path
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("T2L_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm; "gloo" for the dry run
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; running with the {world} rank(s) that exist", file=sys.stderr)
    ranks_seen = 1
    if dist:  # every rank contributes 1 over the data-path backend: the JSON line says how many really took part
        t_seen = torch.ones(1, dtype=torch.int32, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t_seen)
        ranks_seen = int(t_seen.item())

    N_CELLS, N_QUERIES = args.cells, args.queries
    # Kernel durations are taken INSIDE the timed region two ways:
    #  * HIP events on sampled launches (hipExtLaunchKernelGGL start / stop events on the launch stream). Any event pair
    #    costs the stream ~6 us per sampled kernel (measured: marker packets and dispatch-attached events alike), so they
    #    are sampled every 8th launch or sparser — at the driver's --steps 20 that is 3 scan launches;
    #  * the paired scan's own span stamps (s_memrealtime, first workgroup start -> last workgroup end) on EVERY launch,
    #    at no cost to the stream: >= 16 samples whatever --steps is. `roofline` is computed from the HIP events and
    #    carries the stamp average beside it (the two agree to ~1 us: the events include the dispatch's start-up).
    EVENT_EVERY = max(8, args.steps // 16)
    # N_BATCH distinct query batches, rotated step by step (the DB stays resident; a real evaluation never repeats a batch)
    N_BATCH = 4
    db, qs, target = synth.make_retrieval_problem(N_CELLS, N_QUERIES, DIM, seed=1, noise=0.5)
    batches = [(qs, target)]
    for bi in range(1, N_BATCH):
        batches.append(synth.make_queries_for(db, N_QUERIES, seed=100 + bi, noise=0.5))
    eng = Engine(dev)
    searcher = ShardedSearcher(eng)
    d_db = torch.from_numpy(db).cuda()
    d_qs = [torch.from_numpy(np.ascontiguousarray(b[0])).cuda() for b in batches]
    d_q = d_qs[0]
    lo, hi = searcher.set_db_shard(d_db)
    eng.set_option("profile_events", 97)  # outside the timed region: rare (the first samples create the event rings — not in the timed steps)
    eng.set_option("search_mode", args.mode)
    if os.environ.get("T2L_BENCH_TILE_SEL") is not None:  # dev A/B: the paired scan's per-score insertion (0) against the tile-local selection (1, default)
        eng.set_option("search_tile_sel", int(os.environ["T2L_BENCH_TILE_SEL"]))
    if args.nsplit:
        eng.set_option("search_nsplit", args.nsplit)
    N_OUT = 12
    outs = [(torch.empty((N_QUERIES, TOPK), dtype=torch.int32, device="cuda"),
             torch.empty((N_QUERIES, TOPK), dtype=torch.float64, device="cuda")) for _ in range(N_OUT)]

    def step(i):
        if world == 1:  # (ShardedSearcher.search is this call plus the exchange step that one rank does not have)
            return eng.search(d_qs[i % N_BATCH], TOPK, out=outs[i % N_OUT])
        return searcher.search(d_qs[i % N_BATCH], TOPK, out=outs[i % N_OUT])

    # THE CONTRACT REGION (`value`): W warmup steps, then exactly K timed steps between barrier + synchronize on both sides.
    # Nothing runs on the GPU before it but the set-up above — no clock-ramp steps: at the driver's --warmup 5 --steps 20 the
    # GPU is still climbing from its idle clocks (it needs ~40 ms of load to reach the sustained ones), and that is what the
    # headline reports. With --full the sustained rate of the same loop is measured right behind it (`steady_state`, a side field).
    for i in range(args.warmup):
        step(i)
    # forget the samples so far and restart the sampling phase — host-only, the stream keeps running
    eng.set_option("stats_reset", 1)
    eng.set_option("profile_rerank", 0)  # timed region: sampled launches bracket the dominant kernel only; the re-rank is timed below
    eng.set_option("profile_events", EVENT_EVERY)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        idx, sc = step(i)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:  # before anything else runs: later steps of --full reuse the rotated `outs` buffers
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "ids.npy"), idx.cpu().numpy().astype(np.float64))
        np.save(os.path.join(args.dump_outputs, "scores.npy"), sc.cpu().numpy().astype(np.float64))

    ms = 1e3 * elapsed / args.steps
    if args.mode == 2:
        kname, peak, dtype, mult = "scanw_kernel<8, 4>", BF16_MFMA_PEAK_TFLOPS, "bf16x3", 3
    else:
        kname, peak, dtype, mult = ("scanp_kernel<6, 4, true, 1>" if os.environ.get("T2L_BENCH_TILE_SEL", "1") != "0" else "scanp_kernel<6, 4, true, 0>"), BF16_MFMA_PEAK_TFLOPS, "f16", 1  # (merged records + tile-local selection: the default on benign data)
    out = {
        "metric": "coarse-retrieval queries/sec over 11k-cell DB, embed_dim=256; top-1/3/5 recall parity",
        "value": N_QUERIES * args.steps / elapsed,
        "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": dtype, "data": "synthetic",
        "config": {"workload": "KITTI360Pose-sized val DB: N=11259 cells x D=256 resident in HBM, Q=4096 "
                               "precomputed text embeddings per step, top-10 (float64-exact ids)",
                   "n_cells": N_CELLS, "queries_per_step": N_QUERIES, "embed_dim": DIM, "top_k": TOPK,
                   "arithmetic": {0: "f16 MFMA candidate scan (power-of-two scaled operands, f32 accumulate)",
                                  2: "split-bf16 (3 MFMAs per product) candidate scan (f32 accumulate)"}[args.mode]
                                 + " -> float64 re-rank + certificate (ids and scores are the float64 ranking)",
                   "parallelism": f"db-row-shard x{world}" if world > 1 else "single-gpu",
                   "layout": (f"db-row-shard x{world}: shard search -> ONE all_gather of the per-shard top-k -> merge on every rank"
                              if world > 1 else "one resident DB, two launches per step (scan, re-rank)"),
                   "pipelining": "none (stream-ordered steps)",
                   "region": "set-up, then W warmup steps, then K timed steps: no clock-ramp steps before the region"},
        "ranks_seen": ranks_seen,
    }
    if not args.full:
        # the timed region above is the same in both forms (its sampled HIP events included), so `value` means the same;
        # only what --full measures behind it is skipped
        if rank == 0:
            print(format_headline(out), flush=True)
        if dist:
            dist.destroy_process_group()
        return

    scan_region_ms, scan_region_n = eng.kernel_stats("search_scan")
    span_region_ms, span_region_n = eng.kernel_stats("search_scan_span")
    fallbacks = eng.search_fallbacks()
    rescored = eng.search_rescored()
    counters = eng.search_counters()

    # behind the contract region, N=1: the same stream-ordered loop at the sustained clocks — 1,500 untimed steps (~65 ms of load),
    # then 400 timed steps without event pairs (`steady_state`), then 64 steps with every 4th launch bracketed by HIP events
    # (an event pair costs the stream ~6 us, so the K = 20 region itself carries only 2-3 of them): the roofline's kernel
    # duration averages the launches bracketed inside the timed region and these 16.
    RAMP_STEPS = 0 if args.quick else 1500
    steady = None
    scan_ms, scan_n = scan_region_ms, scan_region_n
    scan_post_ms, scan_post_n = None, 0
    if world == 1:
        eng.set_option("profile_events", 0)
        for i in range(RAMP_STEPS):
            step(i)
        if not args.quick:
            torch.cuda.synchronize()
            t0s = time.perf_counter()
            for i in range(400):
                step(i)
            torch.cuda.synchronize()
            ts = (time.perf_counter() - t0s) / 400
            steady = {"steps": 400, "untimed_ramp_steps": RAMP_STEPS, "ms_per_step": ts * 1e3, "queries_per_s": N_QUERIES / ts}
        eng.set_option("profile_events", 4)
        for i in range(16 if args.quick else 64):
            step(args.steps + i)
        torch.cuda.synchronize()
        scan_post_ms, scan_post_n = eng.kernel_stats("search_scan")
        if scan_post_n:
            scan_ms = (scan_region_ms * scan_region_n + scan_post_ms * scan_post_n) / max(1, scan_region_n + scan_post_n)
            scan_n = scan_region_n + scan_post_n
    eng.set_option("profile_rerank", 1)
    span_ms, span_n = eng.kernel_stats("search_scan_span")
    busy_ms, busy_n = eng.kernel_stats("search_scan_busy")
    # the re-rank kernel's duration: the same steps again, every 4th launch bracketed
    eng.set_option("profile_events", 4)
    for i in range(64):
        searcher.search(d_qs[i % N_BATCH], TOPK)
    torch.cuda.synchronize()
    rerank_ms, _ = eng.kernel_stats("search_rerank")
    eng.kernel_stats("search_scan")
    eng.set_option("profile_events", 1)  # the side measurements below bracket every launch

    # parity, outside the timed region: EVERY (id, score) of every rotated batch vs the float64 C oracle (all Q x K pairs)
    parity, max_score_err, recall1, n_checked = True, 0.0, [], 0
    serial_results = {}
    sharded_results = {}
    if world > 1:  # every rank takes part in the exchange of every rotated batch; rank 0 then checks all of them
        for bi in range(N_BATCH):
            ri, rs_ = searcher.search(d_qs[bi], TOPK)
            sharded_results[bi] = (ri.clone(), rs_.clone())
    if rank == 0:
        from oracle import c_oracle
        from concurrent.futures import ThreadPoolExecutor
        nthr = min(32, os.cpu_count() or 1)
        for bi, (bq, btarget) in enumerate(batches):
            gi, gs = searcher.search(d_qs[bi], TOPK) if world == 1 else (None, None)
            if world > 1:
                gi, gs = sharded_results[bi]
            serial_results[bi] = (gi, gs)
            got_i, got_s = gi.cpu().numpy().astype(np.int64), gs.cpu().numpy()
            chunks = np.array_split(np.arange(N_QUERIES), nthr)
            with ThreadPoolExecutor(nthr) as ex:  # ctypes releases the GIL: the scalar oracle runs on nthr host cores
                parts = list(ex.map(lambda c: c_oracle.retrieve_topk(db, bq[c], TOPK), [c for c in chunks if len(c)]))
            ridx = np.concatenate([p_[0] for p_ in parts])
            rsc = np.concatenate([p_[1] for p_ in parts])
            parity = parity and bool(np.array_equal(got_i, ridx))
            max_score_err = max(max_score_err, float(np.abs(got_s - rsc).max()))
            recall1.append(float((got_i[:, 0] == btarget).mean()))
            n_checked += int(ridx.size)

    # N=1, outside the timed region: the same loop PIPELINED (include/t2l.h, t2l_search_join): consecutive steps are independent
    # jobs, so step i runs its scan -> re-rank chain on internal stream i % 3 of the engine and the chains overlap. Reported
    # beside `value` (whose steps are stream-ordered, so that its kernel durations mean what rocprofv3 reports).
    pipelined = None
    if world == 1 and rank == 0 and not args.no_pipelined and not args.quick:
        P_LANES = 3
        eng.set_option("profile_events", 0)
        eng.set_option("search_lanes", P_LANES)
        n_pipe = max(400, args.steps)
        for i in range(1500 + 24):  # (the GPU idled during the CPU oracle above: ramp its clocks again)
            eng.search(d_qs[i % N_BATCH], TOPK, out=outs[i % N_OUT], join=False)
        eng.search_join()
        eng.set_option("stats_reset", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_pipe):
            eng.search(d_qs[i % N_BATCH], TOPK, out=outs[i % N_OUT], join=False)
        eng.search_join()
        torch.cuda.synchronize()
        tp = (time.perf_counter() - t0) / n_pipe
        p_span, _ = eng.kernel_stats("search_scan_span")
        p_busy, _ = eng.kernel_stats("search_scan_busy")
        same = True
        for i in range(n_pipe - N_BATCH, n_pipe):
            same = same and bool(torch.equal(outs[i % N_OUT][0], serial_results[i % N_BATCH][0]) and
                                 torch.equal(outs[i % N_OUT][1], serial_results[i % N_BATCH][1]))
        eng.set_option("search_lanes", 1)
        eng.set_option("profile_events", 1)
        pipelined = {"lanes": P_LANES, "steps": n_pipe, "ms_per_step": tp * 1e3, "queries_per_s": N_QUERIES / tp,
                     "results_equal_stream_ordered": same,
                     "scan_kernel_ms_overlapped_span": p_span, "scan_kernel_ms_gpu_time": p_busy,
                     "note": "kernels of neighbouring steps share the chip: a launch's start -> end span overlaps its neighbours'; "
                             "gpu_time = mean workgroup duration (in-kernel stamps)"}

    # N>1 only, outside the timed region: the OTHER use of N GPUs for a DB this small — replicate the 11.5 MB DB, split the
    # queries, no data-path collective (one all_gather of the results so every rank ends with all [Q,K] rows). Reported
    # beside the north-star row-sharded `value`, never instead of it.
    alt = None
    if world > 1:
        eng_q = Engine(dev)
        qsearch = QueryShardedSearcher(eng_q)
        qsearch.set_db(d_db)
        for _ in range(max(3, args.warmup // 4)):
            qsearch.search(d_q, TOPK)
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_alt = max(10, args.steps // 4)
        for _ in range(n_alt):
            qi, _qs = qsearch.search(d_qs[(args.steps - 1) % N_BATCH], TOPK)
        torch.cuda.synchronize()
        dist.barrier()
        te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        alt = {"layout": "DB replicated on every GPU, queries split across ranks, results all-gathered",
               "queries_per_s": N_QUERIES * n_alt / float(te.item()), "ms_per_step": 1e3 * float(te.item()) / n_alt,
               "ids_equal_row_sharded": bool(torch.equal(qi, idx))}
        eng_q.close()

    # N>1 only, outside the timed region: (i) the WEAK-scaling point of the same layout — every rank holds a full 11,259-row
    # shard of an N x 11,259-row database (BASELINE config 3 says "Full DB": more rows is where row-sharding pays), same Q;
    # (ii) BASELINE config 5 on N ranks: coarse (row-sharded search) + fine (the Q x top-k (pose, cell) pairs split across the
    # ranks, offsets all-gathered: cross_matcher.run_fine's world > 1 decomposition on resident descriptor / hint tables).
    weak = None
    cfg5 = None
    if world > 1:
        from text2loc_amd.sharded import gather_rows, shard_bounds

        def timed_ranks(fn, n):
            for _ in range(3):
                fn()
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                r = fn()
            torch.cuda.synchronize()
            dist.barrier()
            te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            return float(te.item()) / n, r

        try:
            eng_w = Engine(dev)
            sw = ShardedSearcher(eng_w)
            n_total = world * N_CELLS
            rs = np.random.default_rng(1000 + rank)
            shard = torch.from_numpy(synth.unit_rows(rs.standard_normal((N_CELLS, DIM)).astype(np.float32))).cuda()
            sw.set_db_shard(shard, n_total=n_total)  # shard_bounds(n_total, world, rank) == [rank * N, (rank + 1) * N)
            n_w = max(10, args.steps // 2)
            tw, (wi, wsc) = timed_ranks(lambda: sw.search(d_q, TOPK), n_w)
            lo_w = rank * N_CELLS  # the merged result must agree with this rank's own shard wherever it contributed
            li, ls = eng_w.search(d_q, TOPK)
            mine = (wi >= lo_w) & (wi < lo_w + N_CELLS)
            consistent = bool(torch.all(torch.isin(wi[mine], li)))
            weak = {"layout": f"every rank holds {N_CELLS} rows of an {n_total}-row database (rank-seeded unit rows), same {N_QUERIES} queries per step",
                    "rows_total": n_total, "ms_per_step": tw * 1e3, "queries_per_s": N_QUERIES / tw,
                    "row_query_pairs_per_s": N_QUERIES * n_total / tw, "own_rows_in_merged_topk_are_in_local_topk": consistent}
            eng_w.close()
        except Exception as e:
            weak = {"error": repr(e)}
        try:
            eng_f = Engine(dev)
            eng_f.fine_load_weights(synth.make_fine_weights(0), class_embed=True, color_embed=True)
            c_lo, c_hi = shard_bounds(N_CELLS, world, rank)
            cells16 = synth.make_cells(c_hi - c_lo, seed=7000 + rank, min_obj=16, max_obj=16)
            pk = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cells16.items() if k != "counts"}
            desc = gather_rows(eng_f.fine_encode_objects(pk), N_CELLS)      # every rank: the [N,16,128] descriptor table
            hints = torch.nn.functional.normalize(torch.randn(N_QUERIES, 6, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)), dim=-1)
            hi_all = torch.arange(N_QUERIES, dtype=torch.int32, device="cuda").repeat_interleave(TOPK)
            n_pairs = N_QUERIES * TOPK
            p_lo, p_hi = shard_bounds(n_pairs, world, rank)

            def coarse_fine():
                ids, _ = searcher.search(d_q, TOPK)
                ci = ids.reshape(-1)[p_lo:p_hi].contiguous()
                off = eng_f.fine_match(desc, hints, ci, hi_all[p_lo:p_hi].contiguous())
                return gather_rows(off, n_pairs)

            t5, off_all = timed_ranks(coarse_fine, max(5, args.steps // 4))
            cfg5 = {"what": f"coarse (row-sharded search, one all_gather) + fine ({n_pairs} (pose, cell) pairs split over {world} ranks, offsets "
                            "all-gathered) per step; descriptor table built from rank shards with one all_gather",
                    "ms_per_step": t5 * 1e3, "queries_per_s": N_QUERIES / t5, "offsets_finite": bool(torch.isfinite(off_all).all())}
            eng_f.close()
        except Exception as e:
            cfg5 = {"error": repr(e)}

    secondary = {}
    if rank == 0 and world == 1 and not args.no_secondary:
        global _QS
        _QS = qs
        global _QUICK
        _QUICK = bool(args.quick)
        secondary = secondary_measurements(eng)
    if rank == 0:
        n_local = hi - lo
        flops = 2.0 * N_QUERIES * n_local * DIM  # algorithmic FLOPs of one scan launch on this rank's shard
        if world == 1 and not args.quick:
            measure_mfma_ceiling()  # (outside every timed region)
        if world == 1 and args.mode == 0 and not args.quick and not os.environ.get("T2L_BENCH_CHILD"):
            live = measure_traffic_in_run("t2l::scanp_kernel")  # (outside every timed region; ~40 s; None without rocprofv3)
            if live is not None:
                _PMC_LIVE["t2l::" + kname] = live
        out.update({
            "roofline": roofline(kname, peak, mult, flops, scan_ms, scan_n, span_ms, span_n, busy_ms, busy_n),
            "kernels_ms": {"search_scan": scan_ms, "search_rerank": rerank_ms},  # the whole step is these two launches
            "scan_kernel_event_samples": {"inside_the_timed_region": {"kernel_ms": scan_region_ms, "launches_timed": scan_region_n},
                                          "behind_the_timed_region": {"kernel_ms": scan_post_ms, "launches_timed": scan_post_n},
                                          "note": "roofline.kernel_ms averages both sets: an event pair costs the stream ~6 us, so the K = 20 "
                                                  "region carries 3 of them and the same loop continues for 64 steps with every 4th launch bracketed"},
            "scan_span_in_timed_region": {"kernel_ms_in_kernel_span": span_region_ms, "launches": span_region_n},
            "steady_state": steady,
            "pipelined": pipelined,
            "secondary": secondary,
            "parity": {"ids_equal_float64_oracle": parity, "pairs_checked": n_checked,
                       "checked": f"all {N_QUERIES} x {TOPK} (id, score) pairs of {len(recall1)} query batch(es) vs the C oracle",
                       "max_abs_score_err": max_score_err, "recall_at_1_planted": recall1,
                       "exact_fallback_queries_last_step": fallbacks,
                       "first_certificate_failures_last_step": rescored, "counters_last_step": counters},
            "query_batches_rotated": N_BATCH,
        })
        if alt is not None:
            out["alt_query_sharded"] = alt
        if weak is not None:
            out["weak_scaling_point"] = weak
        if cfg5 is not None:
            out["config5_coarse_plus_fine"] = cfg5
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(db, qs)
            out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
            # SURVEY.md §8d "fair CPU" line: the same search as one f32 GEMM + top-k on all host cores (an f32 ranking,
            # not the reference's float64 one) — reported beside the reference-style loop, never as the baseline
            try:
                tq, tdb = torch.from_numpy(qs), torch.from_numpy(db)
                torch.topk(tq @ tdb.t(), TOPK, dim=1)
                t0 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    torch.topk(tq @ tdb.t(), TOPK, dim=1)
                dt = (time.perf_counter() - t0) / reps
                out["cpu_baseline"]["fair_cpu_torch_mm_topk_f32"] = {"queries_per_s": N_QUERIES / dt, "threads": torch.get_num_threads()}
            except Exception as e:
                out["cpu_baseline"]["fair_cpu_torch_mm_topk_f32"] = {"error": repr(e)}
        # the full record goes to a file (and nowhere near stdout: 20 KB on one line once broke the driver's parser);
        # stdout gets one short non-JSON line of side-measurement key figures, then THE line, last, < 4 KB
        try:
            os.makedirs(os.path.dirname(args.detail_out), exist_ok=True)
            with open(args.detail_out, "w") as f:
                json.dump(out, f, indent=1)
            out["detail_file"] = os.path.relpath(args.detail_out, REPO)
        except OSError as e:
            print(f"bench.py: could not write {args.detail_out}: {e}", file=sys.stderr)
        sys.stderr.flush()
        if secondary:
            print(format_secondary(secondary), flush=True)
        print(format_headline(out), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
