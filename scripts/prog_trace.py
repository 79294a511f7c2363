"""Development aid: timeline of one program launch (k_program): when each POTRF job was drawn, could start and ended; the spread
of the TRSM / update jobs; idle gaps on the critical chain.  python scripts/prog_trace.py [case] [opt=val ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import cholesky_amd as ca
from conftest import case_paths

case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
m, o, c, _ = case_paths(case)
plan = ca.Plan(m, o, c)
dev = ca.Device(plan, 0)
for kv in sys.argv[2:]:
    k, v = kv.split("=")
    dev.set_option(k, int(v))
a = dev.new_arena()
for _ in range(3):
    dev.fill(a); dev.factor(a)
dev.sync()
dev.fill(a); dev.sync()
follow_file = os.environ.get("CHOLAMD_TRACE_FOLLOW")
if not follow_file:  # the update jobs' "last stage held" stamps come through the follow trace: a file of our own unless the caller names one
    import tempfile
    follow_file = os.environ["CHOLAMD_TRACE_FOLLOW"] = os.path.join(tempfile.mkdtemp(), "follow.txt")
tr = dev.program_trace(a)
us = tr[:, 1:4] * 0.01
kind = tr[:, 0]
print(f"{case}: {len(tr)} jobs, last end {us[:, 2].max():.1f} us")
names = {0: "POTRF", 10: "POTRF*", 1: "TRSM", 2: "UPD"}
for j in range(len(tr)):
    if kind[j] in (0, 10):
        print(f"  job {j:4d} {names[int(kind[j])]:6s} wg {tr[j, 4]:3d}  drawn {us[j, 0]:7.1f}  start {us[j, 1]:7.1f}  end {us[j, 2]:7.1f}  (busy {us[j, 2] - us[j, 1]:6.1f})")
if os.environ.get("TRACE_JOBS"):  # TRACE_JOBS=lo:hi -- every job of the range
    lo, hi = (int(v) for v in os.environ["TRACE_JOBS"].split(":"))
    for j in range(lo, min(hi, len(tr))):
        print(f"  job {j:4d} kind {int(kind[j]):2d} wg {tr[j, 4]:3d}  drawn {us[j, 0]:7.1f}  start {us[j, 1]:7.1f}  end {us[j, 2]:7.1f}")
for k in (1, 2):
    sel = kind == k
    if sel.any():
        d = us[sel]
        print(f"  {names[k]:5s} jobs {sel.sum():4d}: drawn {d[:, 0].min():6.1f}..{d[:, 0].max():6.1f}  start {d[:, 1].min():6.1f}..{d[:, 1].max():6.1f}  end {d[:, 2].min():6.1f}..{d[:, 2].max():6.1f}  mean busy {np.mean(d[:, 2] - d[:, 1]):5.1f} us, mean wait {np.mean(d[:, 1] - d[:, 0]):5.1f} us")
# per 20 us window: jobs running
for t0 in range(0, int(us[:, 2].max()) + 1, 20):
    run = ((us[:, 1] < t0 + 20) & (us[:, 2] > t0)).sum()
    wait = ((us[:, 0] < t0 + 20) & (us[:, 1] > t0)).sum()
    print(f"  t {t0:4d}-{t0 + 20:4d} us: {run:4d} jobs working, {wait:4d} waiting")

# what each POTRF job waited for last: the job whose signal completed its wait list
jobs, waits = plan.program_jobs(follow=not any(kv == "follow=0" for kv in sys.argv[2:]))
sig_jobs = {}
for j in range(len(jobs)):
    for c in (jobs[j, 5], jobs[j, 6]):
        if c >= 0:
            sig_jobs.setdefault(int(c), []).append(j)
heap_level = {int(plan.tree[h - 1]): h.bit_length() - 1 for h in range(1, plan.nsep + 1)}
def reached(c, v):
    """The job whose signal took counter c to the waited value v: the v-th signaller to end (jobs that signal later do not count towards the wait)."""
    js = sorted(sig_jobs.get(int(c), []), key=lambda q: us[q, 2])
    return js[min(int(v), len(js)) - 1] if js and v > 0 else None


print("critical waits of the POTRF jobs (per counter waited for: the job whose signal took it to the waited value):")
for j in range(len(jobs)):
    if jobs[j, 0] != 0:
        continue
    ws = waits[waits[:, 0] == j]
    worst = None
    for _, c, v in ws:
        last = reached(c, v)
        if last is not None and (worst is None or us[last, 2] > us[worst, 2]):
            worst = last
    if worst is not None:
        print(f"  POTRF job {j} (sep {jobs[j, 1]} level {heap_level[int(jobs[j, 1])]} col0 {jobs[j, 2]}) start {us[j, 1]:6.1f}: last signal from job {worst} kind {jobs[worst, 0]} "
              f"target col-sep {jobs[worst, 1]} row-sep {jobs[worst, 2]}: drawn {us[worst, 0]:6.1f} start {us[worst, 1]:6.1f} end {us[worst, 2]:6.1f}")
        ws2 = waits[waits[:, 0] == worst]
        w2 = None
        for _, c, v in ws2:
            last = reached(c, v)
            if last is not None and (w2 is None or us[last, 2] > us[w2, 2]):
                w2 = last
        if w2 is not None:
            print(f"        ... which waited for job {w2} kind {jobs[w2, 0]} sep {jobs[w2, 1]} aux {jobs[w2, 2]}: drawn {us[w2, 0]:6.1f} start {us[w2, 1]:6.1f} end {us[w2, 2]:6.1f}")

# channel strips (TRSM jobs a follower follows): per pivot block, their start / end against the POTRF job's
print("followed strips (TRSM jobs with a channel) per source pivot block:")
pot = {(int(jobs[j, 1]), int(jobs[j, 2])): j for j in range(len(jobs)) if jobs[j, 0] == 0}
seen = {}
for j in range(len(jobs)):
    if jobs[j, 0] == 1 and jobs[j, 6] >= 0:
        seen.setdefault((int(jobs[j, 1]), int(jobs[j, 2]), int(jobs[j, 6])), []).append(j)
for (sep, col0, ch), js in sorted(seen.items(), key=lambda kv: us[pot[kv[0][:2]], 2]):
    pj = pot[(sep, col0)]
    if heap_level[sep] >= 4 and col0 == 0:
        continue
    print(f"  sep {sep:2d} (level {heap_level[sep]}) col0 {col0:3d} chan {ch:4d}: POTRF start {us[pj, 1]:6.1f} end {us[pj, 2]:6.1f} | strips drawn {min(us[q, 0] for q in js):6.1f} "
          f"start {min(us[q, 1] for q in js):6.1f}..{max(us[q, 1] for q in js):6.1f} end {min(us[q, 2] for q in js):6.1f}..{max(us[q, 2] for q in js):6.1f}")

# update jobs per target panel (column separator): spread of their starts and ends, by source phase order
print("update jobs per target panel:")
for sep in sorted(set(int(v) for v in jobs[jobs[:, 0] == 2, 1]), key=lambda s_: (heap_level[s_], s_), reverse=True):
    js = [j for j in range(len(jobs)) if jobs[j, 0] == 2 and jobs[j, 1] == sep]
    if heap_level[sep] == max(heap_level.values()):
        continue
    line = f"  panel {sep:2d} (level {heap_level[sep]}): {len(js):3d} jobs; "
    # group by queue position clusters (phases): split where job indices jump by > 50
    groups, cur = [], [js[0]]
    for j in js[1:]:
        if j - cur[-1] > 40:
            groups.append(cur); cur = [j]
        else:
            cur.append(j)
    groups.append(cur)
    for gq in groups:
        d = us[gq]
        line += f"[jobs {gq[0]}-{gq[-1]} n={len(gq)} tasks={int(jobs[gq, 4].sum())} drawn {d[:, 0].min():.0f}-{d[:, 0].max():.0f} start {d[:, 1].min():.0f}-{d[:, 1].max():.0f} end {d[:, 2].min():.0f}-{d[:, 2].max():.0f}] "
    print(line)

# update jobs per target panel: from "wave 0 saw the job's last staged wait hold" (slot 0 of the job's extra stamps) to the job's end --
# what a transition pays after the last source of an extend-add job is readable
held = {}
if os.path.exists(follow_file):
    for ln in open(follow_file):
        w = ln.split()
        if len(w) >= 6 and w[2] == "kind" and w[3] == "2" and w[4] == "last-stage-held":
            held[int(w[1])] = float(w[5])
print("update jobs per target panel, last stage held -> job ended (us): jobs stamped / all, min, quartiles, max; the last job to end")
for sep in sorted(set(int(v) for v in jobs[jobs[:, 0] == 2, 1]), key=lambda s_: (heap_level[s_], s_), reverse=True):
    js = [j for j in range(len(jobs)) if jobs[j, 0] == 2 and jobs[j, 1] == sep]
    d = np.array([us[j, 2] - held[j] for j in js if j in held])
    if len(d) == 0:
        print(f"  panel {sep:2d} (level {heap_level[sep]}): {len(js):3d} jobs, none stamped")
        continue
    q = np.percentile(d, [0, 25, 50, 75, 100])
    last = max(js, key=lambda j: us[j, 2])
    tail = f"job {last} held {held[last]:.1f} end {us[last, 2]:.1f}" if last in held else f"job {last} end {us[last, 2]:.1f} (not stamped)"
    print(f"  panel {sep:2d} (level {heap_level[sep]}): {len(d):3d} / {len(js):3d} jobs  {q[0]:5.1f} {q[1]:5.1f} {q[2]:5.1f} {q[3]:5.1f} {q[4]:5.1f}   last to end: {tail}")

# followed strips, column tile by column tile: when the pivot block's POTRF published column tile k and when its strip jobs (first strip of
# each) had put tile k on the channel -- the lag of the first and of the last tile says whether the strips keep the pivot's pace
def _stamps(line, title):
    part = line.split(title)[1].split("|")[0] if title in line else ""
    return {int(kv.split(":")[0]): float(kv.split(":")[1]) for kv in part.split()}


pub, chn = {}, {}
if os.path.exists(follow_file):
    for ln in open(follow_file):
        w = ln.split()
        if len(w) >= 4 and w[2] == "kind" and w[3] == "0":
            pub[int(w[1])] = _stamps(ln, "column published:")
        elif len(w) >= 4 and w[2] == "kind" and w[3] == "1":
            chn[int(w[1])] = _stamps(ln, "column tile on the channel:")
print("followed strips per source pivot block: POTRF published tile k at / latest strip job put tile k on the channel at / lag (us)")
for (sep, col0, ch), js in sorted(seen.items(), key=lambda kv: us[pot[kv[0][:2]], 2]):
    pj = pot[(sep, col0)]
    tiles = sorted(set(pub.get(pj, {})) & set.intersection(*(set(chn.get(q, {})) for q in js)))
    if not tiles:
        continue
    p = [pub[pj][k] for k in tiles]
    c = [max(chn[q][k] for q in js) for k in tiles]
    print(f"  sep {sep:2d} (level {heap_level[sep]}) col0 {col0:3d} jobs {js[0]}-{js[-1]}: tiles {tiles[0]}..{tiles[-1]}  lag first {c[0] - p[0]:4.1f} last {c[-1] - p[-1]:4.1f}\n"
          f"      published  {' '.join(f'{v:6.1f}' for v in p)}\n      on channel {' '.join(f'{v:6.1f}' for v in c)}")

# TRACE_WAITS=lo:hi -- per job of the range: every wait (in list order = stage order) with the time its counter was complete
if os.environ.get("TRACE_WAITS"):
    lo, hi = (int(v) for v in os.environ["TRACE_WAITS"].split(":"))
    print("waits per job (counter: value needed, completed at = end of the last job signalling it; channel counters are raised by strips column by column: shown as the strips' end):")
    chan_jobs = {}
    for j in range(len(jobs)):
        if jobs[j, 0] == 1 and jobs[j, 6] >= 0:
            for t in range(32):
                chan_jobs.setdefault(int(jobs[j, 6]) + t, []).append(j)
    for j in range(lo, min(hi, len(jobs))):
        ws = waits[waits[:, 0] == j]
        line = f"  job {j} kind {jobs[j, 0]} sep {jobs[j, 1]} aux {jobs[j, 2]} tasks {jobs[j, 4]}: drawn {us[j, 0]:.1f} start {us[j, 1]:.1f} end {us[j, 2]:.1f} |"
        for _, c, v in ws:
            js = sig_jobs.get(int(c), []) or chan_jobs.get(int(c), [])
            t = max((us[q, 2] for q in js), default=-1.0)
            line += f" c{c}>={v}@{t:.1f}"
        print(line)

# followers: the four instants of a transition -- the last followed column tile on the channel, the wait for the own tiles over, the first column
# started -- and where the own tiles go in (Plan.program_follow_own under the option given on the command line)
own_opt = next((int(kv.split("=")[1]) for kv in sys.argv[2:] if kv.startswith("follow_own=")), -1)
tail_opt = next((int(kv.split("=")[1]) for kv in sys.argv[2:] if kv.startswith("follow_tail=")), -1)
place = {f["job"]: f for f in plan.program_follow_own(own_opt, follow_tail=tail_opt)}
heap_of = {int(plan.tree[h - 1]): h for h in range(1, plan.nsep + 1)}
fol = {}
if os.path.exists(follow_file):
    for ln in open(follow_file):
        w = ln.split()
        if len(w) >= 8 and w[2] == "kind" and w[3] == "0" and w[4] == "items":
            fol[int(w[1])] = (float(w[7]), _stamps(ln, "rounds:"), _stamps(ln, "column started:"))
print("followers (us): job, items, tile columns, own tiles at | last followed tile on the channel, last round taken, own-tiles wait over, first column started | wait over -> start")
for j in sorted(fol):
    if j not in place or place[j]["n_wait"] == 0:
        continue
    over, rounds, started = fol[j]
    sep, col0 = int(jobs[j, 1]), int(jobs[j, 2])
    # the sources: the strips of the block before (a later column block), of the children's rows of this separator (a first block); a block with two
    # channels has the one to its own next block first
    srcs = []
    for (s2, c2, ch), js in seen.items():
        chans = sorted(k[2] for k in seen if k[:2] == (s2, c2))
        has_next = any(k[0] == s2 and k[1] > c2 for k in pot)
        below = ch == chans[0] and has_next and (len(chans) == 2 or heap_of[s2] == 1)
        if col0 > 0 and s2 == sep and below and c2 == max(k[1] for k in pot if k[0] == sep and k[1] < col0):
            srcs += js
        if col0 == 0 and heap_of[s2] // 2 == heap_of[sep] and not below:
            srcs += js
    on_chan = max((max(chn[q].values()) for q in srcs if chn.get(q)), default=float("nan"))
    f = place[j]
    start = started.get(0, float("nan"))
    print(f"  job {j:4d} items {f['n_ext']:2d} T {f['T']:2d} own at {f['own_at']:2d}{' (last)' if f['own_at'] == f['n_ext'] else '':7s} | {on_chan:6.1f} {max(rounds.values(), default=float('nan')):6.1f} "
          f"{over:6.1f} {start:6.1f} | {start - over:4.1f}   wait over {'after' if over > on_chan else 'before'} the last followed tile")
