"""Parent-against-new A/B of the streaming attention forward: does writing pv_attn_stream_kernel and pv_attn_stream_var_kernel
as one body cost time?  Several builds of the library in one process through ctypes, as scripts/raster_ab.py.

    python scripts/stream_refactor_ab.py --parent DIR [--rounds 15] [--iters 200] [--out profiles/stream_refactor_ab.json]

DIR holds the PARENT commit's libpeekvit_hip.so and libpeekvit_hip_f16.so; the new build is the in-tree one.  Three handles per operand build:
the parent, a second load of the parent (a copy of the file: dlopen returns the first handle for the same path) and the new library.  The second
load is the method's noise: the same code timed as if it were another build.  Per round every handle launches `iters` times between two device
events, the three in an order that rotates from round to round; a case's figure is the median over the rounds.

Cases (the shapes the project benchmarks):
  * the training forward with lse at rows 401 and 785, dh 64, 4 heads, batch 256 (scripts/bench_long_train.py), plain / W / DROP;
  * the ragged forward on the rows the compacting forward hands it at 160 px and 224 px (scripts/bench_residual_sparse.py: small dims, batch 2048 /
    512): seeded segment lengths between 209 (the shortest the streaming kernel is given) and the image's 402 / 786 rows, the longest first, with
    multiplicities;
  * the inference forward without lse at S = 577, dh 64, 12 heads, batch 64 (pv_attention_bf16).
Before timing, every case's outputs of the new library are compared with the parent's, bit for bit.

A case fails when new / parent - 1 exceeds the largest |parent2 / parent - 1| of the run."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, I64, F32, U64 = C.c_void_p, C.c_int64, C.c_float, C.c_uint64
SIGS = {"pv_attention_stream_lse_bf16": [P, P, P, I64, I64, I64, I64, P, P],
        "pv_attention_stream_lse_w_bf16": [P, P, P, I64, I64, I64, I64, F32, P, P],
        "pv_attention_stream_lse_drop_bf16": [P, P, P, I64, I64, I64, I64, F32, U64, U64, P, P],
        "pv_attention_varlen_w_stream_bf16": [P, P, P, P, I64, I64, I64, I64, P, P],
        "pv_attention_bf16": [P, P, I64, I64, I64, I64, P, P]}


def load(path):
    lib = C.CDLL(path)
    for name, args in SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="directory with the parent commit's two libraries")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_refactor_ab.json"))
    a = ap.parse_args()

    import torch
    from peekvit_amd import _build
    assert torch.cuda.is_available(), "needs a MI355X"
    dev = torch.device("cuda:0")
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    tmp = tempfile.mkdtemp()
    results = {}
    try:
        for mode, name, new_path in (("bf16", "libpeekvit_hip.so", _build.LIB), ("f16", "libpeekvit_hip_f16.so", _build.LIB_F16)):
            second = os.path.join(tmp, "second_" + name)
            shutil.copy(os.path.join(a.parent, name), second)
            libs = {"parent": load(os.path.join(a.parent, name)), "parent2": load(second), "new": load(new_path)}
            dt = torch.float16 if mode == "f16" else torch.bfloat16
            g = torch.Generator().manual_seed(0)

            def qkv_rows(rows, H, dh):
                t = torch.randn(rows, 3 * H * dh, generator=g)
                t[:, :H * dh] *= dh ** -0.5
                return t.to(dt).to(dev)

            cases = {}
            for S in (401, 785):
                B, H, dh = 256, 4, 64
                qkv = qkv_rows(B * S, H, dh)
                out = torch.zeros((B * S, H * dh), dtype=dt, device=dev)
                lse = torch.zeros((B, H, S), dtype=torch.float32, device=dev)
                ptrs = (qkv.data_ptr(), out.data_ptr(), lse.data_ptr())
                cases[f"lse/S{S}"] = (lambda lib, p=ptrs, B=B, S=S, H=H, dh=dh: lib.pv_attention_stream_lse_bf16(*p, B, S, H, dh, None, stream), (out, lse), (qkv,))
                cases[f"lse_w/S{S}"] = (lambda lib, p=ptrs, B=B, S=S, H=H, dh=dh: lib.pv_attention_stream_lse_w_bf16(*p, B, S, H, dh, 1.6094379, None, stream), (out, lse), (qkv,))
                cases[f"lse_drop/S{S}"] = (lambda lib, p=ptrs, B=B, S=S, H=H, dh=dh: lib.pv_attention_stream_lse_drop_bf16(*p, B, S, H, dh, 0.1, 7, 3, None, stream),
                                           (out, lse), (qkv,))
            for px, rows, B in ((160, 402, 2048), (224, 786, 512)):
                H, dh = 4, 64
                lens = torch.randint(209, rows + 1, (B,), generator=g)
                lens[0] = rows
                seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).to(torch.int32).to(dev)
                R = int(lens.sum())
                qkv = qkv_rows(R, H, dh)
                mult = torch.randint(1, 198, (R,), generator=g)
                mult[torch.rand(R, generator=g) < 0.6] = 1
                lm = torch.log(mult.float()).to(dev)
                out = torch.zeros((R, H * dh), dtype=dt, device=dev)
                ptrs = (qkv.data_ptr(), out.data_ptr(), seg.data_ptr(), lm.data_ptr())
                cases[f"ragged/{px}px"] = (lambda lib, p=ptrs, B=B, rows=rows, H=H, dh=dh: lib.pv_attention_varlen_w_stream_bf16(*p, B, rows, H, dh, None, stream),
                                           (out,), (qkv, seg, lm))
            B, S, H, dh = 64, 577, 12, 64
            qkv = qkv_rows(B * S, H, dh)
            out = torch.zeros((B * S, H * dh), dtype=dt, device=dev)
            ptrs = (qkv.data_ptr(), out.data_ptr())
            cases["infer/S577"] = (lambda lib, p=ptrs: lib.pv_attention_bf16(*p, 64, 577, 12, 64, None, stream), (out,), (qkv,))

            for cname, (call, outs, _keep) in cases.items():
                want = None
                for tag in ("parent", "new"):                       # same bits first, and the warm-up of both code objects
                    for t in outs:
                        t.zero_()
                    rc = call(libs[tag])
                    assert rc == 0, (cname, tag, rc)
                    torch.cuda.synchronize()
                    got = [t.clone() for t in outs]
                    if want is None:
                        want = got
                    else:
                        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(want, got)), f"{mode} {cname}: bits differ"
                call(libs["parent2"])
                torch.cuda.synchronize()
                times = {tag: [] for tag in libs}
                order = list(libs)
                for r in range(a.rounds):
                    for tag in order[r % 3:] + order[:r % 3]:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            call(libs[tag])
                        e1.record()
                        torch.cuda.synchronize()
                        times[tag].append(e0.elapsed_time(e1) / a.iters)
                med = {tag: statistics.median(v) for tag, v in times.items()}
                results[f"{mode}/{cname}"] = {"parent_ms": round(med["parent"], 4), "parent2_ms": round(med["parent2"], 4), "new_ms": round(med["new"], 4),
                                              "new_over_parent": round(med["new"] / med["parent"], 4),
                                              "parent2_over_parent": round(med["parent2"] / med["parent"], 4)}
                print(f"{mode}/{cname}", results[f"{mode}/{cname}"], flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    spread = max(abs(r["parent2_over_parent"] - 1.0) for r in results.values())
    slower = {k: r["new_over_parent"] for k, r in results.items() if r["new_over_parent"] - 1.0 > spread}
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "same_bits": True, "cases": results,
           "parent_vs_parent_spread": round(spread, 4), "slower_than_spread": slower}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"parent_vs_parent_spread": doc["parent_vs_parent_spread"], "slower_than_spread": slower}))
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
