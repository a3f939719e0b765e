"""min / median / max duration of every se_tail, in_apply_pack, gem_neck, se_finalize and stem_split launch position, and of the whole forward, over
the eight forwards before the last of a rocprofv3 --kernel-trace database (tools/time_pass.py, tools/profile_small_batch.py):
    python3 tools/probes/launch_spread.py <dir>/p_results.db"""
import re, sqlite3, sys
c = sqlite3.connect(sys.argv[1])
tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
rows = c.execute(f"select s.kernel_name,d.start,d.end from {kd} d join {ks} s on d.kernel_id=s.id order by d.start").fetchall()
starts = [i for i, r in enumerate(rows) if "stem_split" in r[0]]
fw = [rows[a:b] for a, b in zip(starts[-9:-1], starts[-8:])]     # eight whole forwards before the last
per = {}
for f in fw:
    cnt = {}
    for n, s, e in f:
        key = next((k for k in ("se_tail", "in_apply_pack", "gem_neck", "se_finalize", "stem_split") if k in n), None)
        if key:
            cnt[key] = cnt.get(key, 0) + 1
            per.setdefault((key, cnt[key]), []).append((e - s) / 1e3)
    per.setdefault(("forward", 1), []).append((f[-1][2] - f[0][1]) / 1e3)
tot = {}
for (k, i), v in sorted(per.items()):
    v = sorted(v)
    print("SPREAD %-14s #%d  min %7.1f  med %7.1f  max %7.1f us  (%d)" % (k, i, v[0], v[len(v) // 2], v[-1], len(v)))
    tot[k] = tot.get(k, 0) + v[len(v) // 2]
print("SPREAD totals (medians): " + "  ".join("%s %.1f" % kv for kv in sorted(tot.items())))
