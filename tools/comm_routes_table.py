"""Table of tests/test_learner_comm_routes_gpu.py's measurements (profiles/comm_routes_oracle.txt) from the two files the test writes
next to the gradient-error log of tests/util.py: comm_routes_oracle.jsonl (worst gradient ratio, decision statistics per case) and
comm_routes_dispatch.jsonl (the C-ABI entries each update went through).

    python tools/comm_routes_table.py [directory of the jsonl files] > table.txt"""
import json
import os
import sys
import textwrap


def _rows(path):
    rows = {}
    if os.path.exists(path):
        with open(path) as f:
            for line in f:
                r = json.loads(line)
                rows[r["case"]] = r         # a case run twice: the last run counts
    return list(rows.values())


def main(where):
    oracle, dispatch = _rows(os.path.join(where, "comm_routes_oracle.jsonl")), _rows(os.path.join(where, "comm_routes_dispatch.jsonl"))
    upd, step = [r for r in oracle if r["kind"] == "update"], [r for r in oracle if r["kind"] == "step"]
    out = []
    head = f"{'case':34}{'worst ratio':>12}  {'parameter':28}{'argmax':>7}{'margin':>9}{'relu':>14}{'margin':>9}"
    out += [head, "-" * len(head)]
    for r in upd:
        out.append(f"{r['case']:34}{r['worst_grad_ratio']:12.3f}  {r['worst_grad']:28}{r['argmax']:7d}{r['argmax_margin']:9.1e}"
                   f"{str(r['relu']) + '/' + str(r['relu_total']):>14}{r['relu_margin']:9.1e}")
    out.append("")
    head = f"{'case':34}{'worst ratio':>12}  {'parameter (talk kernels)':52}{'relu':>14}{'margin':>9}{'rows redrawn':>14}"
    out += [head, "-" * len(head)]
    for r in step:
        out.append(f"{r['case']:34}{r['worst_grad_ratio']:12.3f}  {r['worst_grad']:52}{str(r['relu']) + '/' + str(r['relu_total']):>14}"
                   f"{r['relu_margin']:9.1e}{r['kink_rows_redrawn']:14d}")
    out.append("")
    if dispatch:
        common = set.intersection(*(set(r["called"]) for r in dispatch))
        out.append("C-ABI entries called by every update:")
        out += textwrap.wrap(" ".join(sorted(common)), 138, initial_indent="  ", subsequent_indent="  ")
        for r in dispatch:
            extra = sorted(set(r["called"]) - common)
            out += textwrap.wrap(f"{r['case']}: + " + (" ".join(extra) if extra else "(nothing)"), 138, initial_indent="  ",
                                 subsequent_indent="      ")
        out += ["", "uavgnn_gemm_nt_x3 calls as rows x K x outputs (the time-batched encoder's over (T + 1) N and T N rows, the steps' over N):"]
        for r in dispatch:
            out += textwrap.wrap(f"{r['case']}: " + " ".join("x".join(map(str, s)) for s in r.get("gemm_nt_x3", [])), 138,
                                 initial_indent="  ", subsequent_indent="      ")
    print("\n".join(out))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:       # where the test wrote them: the directory of the gradient-error log
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
        from tests.util import _GRAD_LOG
        main(os.path.dirname(_GRAD_LOG))
