"""LDS bank conflicts of csrc/cdlong_kernels.h, enumerated (no GPU): every fused pass, the lone radix-2 stage and the linear load and
store of the tile, for every wave, in the column layout of passes A and C (N1 = 2^7 .. 2^9, 16 columns) and in the row layout of pass B
(N2 = 2^7 .. 2^11, max(1, 1024 / N2) rows per work-group).  The rule: ds_read_b64 is served in two groups of 32
lanes over 32 slots of 8 bytes, ds_write_b64 in four groups of 16 lanes over 16 slots; the degree printed is the most distinct
addresses that meet on one slot within a group, as (reads, writes) per pass: 1 is conflict-free.  The forward and the inverse
transforms touch the same elements per work item, so one enumeration serves both."""

def sw(i): return i ^ (21 if i & 32 else 0) ^ (31 if i & 64 else 0)
def par(i):
    p = i >> 1; p ^= p >> 4; p ^= p >> 2; p ^= p >> 1; return p & 1
def at(col, i, t, ln): return ((i ^ par(i)) << 4) | t if col else (t << ln) | sw(i)
def item(col, w, lg): return (w >> 4, w & 15) if col else (w & ((1 << lg) - 1), w >> lg)

def degree(addrs, group, slots):
    # addrs: per lane (len 64) address or None; worst over groups of `group` lanes of distinct addresses per slot
    worst = 0
    for g in range(0, 64, group):
        per = {}
        for a in addrs[g:g + group]:
            if a is None: continue
            per.setdefault(a % slots, set()).add(a)
        if per: worst = max(worst, max(len(s) for s in per.values()))
    return worst

def passes(col, ln, lt):
    n = 1 << ln
    out = []
    lh = ln - 1
    stages = []
    while lh >= 1:
        stages.append(lh); lh -= 2
    for lh in stages:
        lq = lh - 1; hh = 1 << lq
        acc = []
        for w in range((n >> 2) << lt):
            q, t = item(col, w, ln - 2)
            p = q & (hh - 1); a = ((q >> lq) << (lq + 2)) | p
            acc.append([at(col, a + k * hh, t, ln) for k in range(4)])
        out.append(("fused h=2^%d" % lh, acc))
    if ln & 1:
        acc = []
        for w in range((n >> 1) << lt):
            q, t = item(col, w, ln - 1)
            acc.append([at(col, 2 * q, t, ln), at(col, 2 * q + 1, t, ln)])
        out.append(("radix-2", acc))
    return out

def report(name, acc):
    # acc: list over work items of lists of addresses (one per instruction)
    rd = wr = 0
    for w0 in range(0, len(acc), 64):
        chunk = acc[w0:w0 + 64]
        for k in range(len(chunk[0])):
            lanes = [c[k] for c in chunk] + [None] * (64 - len(chunk))
            rd = max(rd, degree(lanes, 32, 32)); wr = max(wr, degree(lanes, 16, 16))
    return rd, wr

for ln in (7, 8, 9):
    res = [(nm,) + report(nm, acc) for nm, acc in passes(True, ln, 4)]
    lin = [[at(True, w >> 4, w & 15, ln)] for w in range((1 << ln) * 16)]
    print("COL N1=2^%d" % ln, res, "load/store", report("lin", lin))
for ln in (7, 8, 9, 10, 11):
    lr = 10 - ln if ln < 10 else 0
    res = [(nm,) + report(nm, acc) for nm, acc in passes(False, ln, lr)]
    lin = [[at(False, w & ((1 << ln) - 1), w >> ln, ln)] for w in range((1 << ln) << lr)]
    print("ROW N2=2^%d" % ln, res, "load/store", report("lin", lin))
