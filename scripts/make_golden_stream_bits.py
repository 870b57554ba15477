"""Record tests/golden/stream_attention_bits.json: the sha256 of every buffer the streaming attention kernels write, per case of
tests/stream_bits_ref.py and per operand build, on the MI355X.  Run it on the build whose bits are to be pinned, BEFORE changing the kernels:

    python scripts/make_golden_stream_bits.py [--out PATH]

The file holds only hashes, shapes and seeds; tests/test_hip_stream_bits.py recomputes every case and compares."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "stream_attention_bits.json"))
    args = ap.parse_args()
    import torch
    import stream_bits_ref as SB
    assert torch.cuda.is_available(), "needs a MI355X"
    res = SB.run_all(torch.device("cuda:0"))
    again = SB.run_all(torch.device("cuda:0"))
    assert res == again, "two runs of the same build differ: these kernels are meant to be deterministic"
    for mode in SB.MODES:
        assert len(res[mode]) == SB.N_CASES, (mode, len(res[mode]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {sum(len(v) for v in res.values())} cases ({', '.join(SB.MODES)})")


if __name__ == "__main__":
    main()
