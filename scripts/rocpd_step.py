"""Cut one steady-state training step out of a rocprofv3 rocpd SQLite DB.

A step is everything dispatched after one adam_kernel ends up to and
including the next adam_kernel. Prints each dispatch's start offset from
the previous Adam's end, its duration, its hardware queue and its name,
then the dispatch count. Usage:
  python scripts/rocpd_step.py <results.db> [steps_from_end]
steps_from_end (default 10) picks the step, counted back from the last.
"""
import sqlite3
import sys


def main():
    db = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    con = sqlite3.connect(db)
    cur = con.cursor()
    tables = [r[0] for r in cur.execute(
        "SELECT name FROM sqlite_master WHERE type='table'")]
    disp = next((t for t in tables if "kernel_dispatch" in t), None)
    if disp is None:
        print("tables:", tables)
        sys.exit(1)
    cols = [r[1] for r in cur.execute(f"PRAGMA table_info({disp})")]
    qcol = next((c for c in ("queue_id", "queue", "stream_id") if c in cols),
                "0")
    if "name" in cols:
        q = f"SELECT name, {qcol}, start, end FROM {disp} ORDER BY start"
    else:
        sym = next((t for t in tables if "kernel_symbol" in t), None)
        scols = [r[1] for r in cur.execute(f"PRAGMA table_info({sym})")]
        name_c = ("display_name" if "display_name" in scols
                  else "kernel_name" if "kernel_name" in scols else "name")
        key = ("kernel_id" if "kernel_id" in cols else "kernel_symbol_id")
        skey = ("id" if "id" in scols else "kernel_id")
        q = (f"SELECT s.{name_c}, d.{qcol}, d.start, d.end FROM {disp} d "
             f"JOIN {sym} s ON d.{key}=s.{skey} ORDER BY d.start")
    rows = list(cur.execute(q))
    adams = [i for i, r in enumerate(rows) if "adam_kernel" in r[0]]
    if len(adams) < back + 2:
        print(f"only {len(adams)} adam_kernel dispatches")
        sys.exit(1)
    lo, hi = adams[-back - 2], adams[-back - 1]
    t0 = rows[lo][3]
    queues = {}
    print(f"{'queue':>5} {'start_us':>9} {'dur_us':>7}  kernel")
    for name, qid, s, e in rows[lo + 1:hi + 1]:
        qn = queues.setdefault(qid, len(queues) + 1)
        nm = name.split("(")[0][:60]
        print(f"{'q%d' % qn:>5} {(s - t0) / 1e3:>+9.1f} {(e - s) / 1e3:>7.1f}  {nm}")
    print(f"dispatches in the step: {hi - lo}; "
          f"adam end to adam end: {(rows[hi][3] - t0) / 1e3:.1f} us")


if __name__ == "__main__":
    main()
