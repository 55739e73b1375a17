"""Seeded genomes with repeat structure, for the tests of the pair path and of the k-mer prefilter.

The random genomes of tools/synth_genomes.py hold a k-mer once (under 1 % of the 11-mers of a 10 kbp genome occur twice, no
21-mer does), so the rules that decide WHICH occurrence the parse takes never run on them.  The genomes here are laid out
from pieces: dispersed repeat families (exact, diverged and reverse-complemented copies), tandem arrays (units of 2-60 bp,
and of exactly 16, 32 and 64 bp: the word and wave widths), homopolymers, an exact segmental duplication, a hairpin and a
terminal repeat, in a random backbone.  The pieces are made first and the backbone gets what is left of the target length,
so a genome has exactly the length asked for.  A relative is made piece by piece, so that the places of its repeat copies
are known: the backbone mutates freely, the copies of a repeat diverge in concert (a relative stays as repeat-rich as its
ancestor), it gains and loses copies of a family, its tandem arrays expand and contract, one block is translocated, and N
runs can be put next to and inside a repeat copy.

Everything draws from synth_genomes.Stream, so the bytes depend on the seed alone (tests/test_repeats.py holds a checksum of
every named set).  Caps, to keep a pair from going quadratic: a homopolymer 200 bp, a tandem array 2.5 kbp, a family 24
copies."""
import zlib

import numpy as np

import synth_genomes as SG
import util as U

MAX_HOMO, MAX_ARRAY, MAX_COPIES = 200, 2500, 24
WIDTH_UNITS = (16, 32, 64)


def rc(x):
    """Reverse complement of symbol codes; an N stays an N (code 5)."""
    x = np.asarray(x, dtype=np.uint8)
    out = (3 - x[::-1]).astype(np.uint8)
    out[x[::-1] > 3] = 5
    return out


def _rnd(st, n):
    return (st.u64(n) % np.uint64(4)).astype(np.uint8)


class Layout:
    """A genome as its pieces in text order: (kind, id, codes).  kind: "bb" backbone, "fam" a family copy (id = family),
    "tan" a tandem array (id = array; units[id] is its unit), "homo", "dup", "pal", "term"."""

    def __init__(self, pieces, units, elements):
        self.pieces, self.units, self.elements = pieces, units, elements

    def codes(self):
        return np.ascontiguousarray(np.concatenate([p[2] for p in self.pieces])) if self.pieces else np.zeros(0, np.uint8)

    def spans(self, kinds=("fam", "dup")):
        """(start, end) of every piece of the kinds, in text order."""
        out, o = [], 0
        for kind, _, x in self.pieces:
            if kind in kinds:
                out.append((o, o + len(x)))
            o += len(x)
        return out


def structured_layout(st, L, share=0.45):
    """The layout of one structured genome of exactly L symbols.  About `share` of it is repeat content; element and array
    lengths are the sketch's at 12 kbp and scale with L below that (down to genomes of 50 bp) and, for the families and
    the duplication, above it."""
    f = L / 12000.0
    small, big = min(1.0, f), max(1.0, f)
    sc = lambda lo, hi, s: (max(1, int(lo * s)), max(2, int(hi * s)))
    budget = total = int(share * L)                                # (every kind gets a bounded part of it, so every kind fits)
    parts, units, elements = [], [], []

    def take(kind, ident, x):
        nonlocal budget
        if len(x) == 0 or len(x) > budget:
            return False
        parts.append((kind, ident, np.ascontiguousarray(x, dtype=np.uint8)))
        budget -= len(x)
        return True

    lo, hi = sc(1000, 3000, small * min(big, 8.0))                 # segmental duplication, exact: a fifth of the budget at most
    d = _rnd(st, min(st.randint(lo, hi), max(1, total // 10)))
    take("dup", 0, d)
    take("dup", 0, d)
    # one tandem array of a width unit and two of any unit, 5-40 units each
    for t in range(3):
        unit = WIDTH_UNITS[st.randint(0, 2)] if t == 0 else st.randint(2, 60)
        unit = max(1, min(unit, int(unit * small) if small < 0.5 else unit))
        reps = st.randint(5, 40)
        reps = max(2, min(reps, MAX_ARRAY // unit, max(2, total // 12 // unit)))
        u = _rnd(st, unit)
        units.append(u)
        take("tan", len(units) - 1, np.tile(u, reps))
    for h in range(4):                                             # homopolymers: one of them 60 bp or more
        lo, hi = sc(12, 120, small)
        n = min(st.randint(lo, hi), MAX_HOMO)
        if h == 0 and small == 1.0:
            n = max(n, 60)
        take("homo", 0, np.full(n, st.randint(0, 3), np.uint8))
    lo, hi = sc(100, 600, small)                                   # hairpin: s + rc(s)
    s = _rnd(st, min(st.randint(lo, hi), max(1, total // 20)))
    take("pal", 0, np.concatenate([s, rc(s)]))
    lo, hi = sc(200, 800, small)                                   # direct or inverted terminal repeat
    t = _rnd(st, min(st.randint(lo, hi), max(1, total // 20)))
    t2 = t if st.one() < 0.5 else rc(t)
    term = len(t) * 2 <= budget
    if term:
        budget -= 2 * len(t)
    fam = 0
    while budget > 0.02 * L and fam < 400:                         # dispersed repeat families until the share is spent
        lo, hi = sc(300, 1500, small * min(big, 8.0))
        e = _rnd(st, min(st.randint(lo, hi), max(1, budget // 3)))
        elements.append(e)
        copies = min(st.randint(2, 6 if big < 4 else 16), MAX_COPIES)
        placed = 0
        for c in range(copies):
            x = e if (c == 0 or st.one() < 0.4) else SG.mutate(e, 0.03 * st.one(), st)
            if st.one() < 0.3:
                x = rc(x)
            if not take("fam", fam, x):
                break
            placed += 1
        if placed < 2:                                              # a family of one copy is no repeat: close with an exact second
            if placed == 1:
                parts.append(("fam", fam, e.copy()))
                budget -= len(e)
            break
        fam += 1
    used = sum(len(p[2]) for p in parts) + (2 * len(t) if term else 0)
    bb = _rnd(st, max(0, L - used))
    # the pieces go between backbone chunks, in a seeded order
    order = np.argsort(st.u64(len(parts)), kind="stable") if parts else []
    cuts = np.sort(st.u64(len(parts)) % np.uint64(len(bb) + 1)).astype(np.int64) if parts else []
    pieces, prev = [], 0
    for k, c in zip(order, cuts):
        pieces.append(("bb", 0, bb[prev:c]))
        pieces.append(parts[int(k)])
        prev = int(c)
    pieces.append(("bb", 0, bb[prev:]))
    if term:
        pieces = [("term", 0, t)] + pieces + [("term", 0, t2)]
    return Layout(pieces, units, elements)


def structured(st, L, **kw):
    return structured_layout(st, L, **kw).codes()


def relative_layout(lay, st, d):
    """A relative at divergence d, piece by piece.  The backbone pieces are mutated on their own (SG.mutate: substitutions
    and indels).  The repeats diverge from the ancestor in concert, as repeats that keep being copied do: the copies of one
    family (and the two of the duplication, the terminal repeat) are mutated from one stream state each, so copies that
    were equal stay equal to each other; a tandem array is its mutated unit tiled; the hairpin is s' + rc(s'); a
    homopolymer changes its length.  One family gains a copy and one loses one; one tandem array expands and one contracts
    by whole units."""
    fam_ids = sorted({p[1] for p in lay.pieces if p[0] == "fam"})
    tan_ids = sorted({p[1] for p in lay.pieces if p[0] == "tan"})
    gain = fam_ids[st.randint(0, len(fam_ids) - 1)] if fam_ids else -1
    loss = fam_ids[st.randint(0, len(fam_ids) - 1)] if fam_ids else -1
    grow = tan_ids[st.randint(0, len(tan_ids) - 1)] if tan_ids else -1
    shrink = tan_ids[st.randint(0, len(tan_ids) - 1)] if tan_ids else -1
    if loss == gain and len(fam_ids) > 1:                             # (a gain and a loss of one family would cancel)
        loss = fam_ids[(fam_ids.index(gain) + 1) % len(fam_ids)]
    elif loss == gain:
        loss = -1
    if shrink == grow and len(tan_ids) > 1:
        shrink = tan_ids[(tan_ids.index(grow) + 1) % len(tan_ids)]
    elif shrink == grow:
        shrink = -1
    seeds = {}

    def concerted(key, x):
        if key not in seeds:
            seeds[key] = int(st.u64(1)[0])
        return SG.mutate(x, d, SG.Stream(seeds[key]))

    out, lost = [], False
    changes = dict(gained=None, lost=None, units={})            # what was done: families by id, arrays id -> (units before, after)
    for kind, ident, x in lay.pieces:
        if kind == "fam" and ident == loss and not lost and sum(1 for p in lay.pieces if p[0] == "fam" and p[1] == ident) > 2:
            lost = True
            changes["lost"] = ident
            continue
        if kind == "tan":
            u = concerted(("tan", ident), lay.units[ident])
            before = reps = len(x) // len(lay.units[ident])
            if ident == grow:
                reps += st.randint(1, 6)
            elif ident == shrink:
                reps = max(2, reps - st.randint(1, 6))
            reps = max(1, min(reps, MAX_ARRAY // max(1, len(u))))
            y = np.tile(u, reps) if len(u) else x
            changes["units"][ident] = (before, reps if len(u) else before)
        elif kind == "homo":
            y = np.full(max(1, min(MAX_HOMO, len(x) + st.randint(-5, 5))), x[0], np.uint8)
        elif kind == "pal":
            h = concerted(("pal", ident), x[:len(x) // 2])
            y = np.concatenate([h, rc(h)])
        elif kind == "bb":
            y = SG.mutate(x, d, st) if len(x) else x
        else:
            y = concerted((kind, ident), x)
        out.append((kind, ident, np.ascontiguousarray(y)))
    if gain >= 0 and gain < len(lay.elements) and sum(1 for p in out if p[0] == "fam" and p[1] == gain) < MAX_COPIES:
        bbs = [k for k, p in enumerate(out) if p[0] == "bb" and len(p[2]) > 1]
        if bbs:
            k = bbs[st.randint(0, len(bbs) - 1)]
            a = st.randint(1, len(out[k][2]) - 1)
            x = out[k][2]
            out[k:k + 1] = [("bb", 0, x[:a]), ("fam", gain, concerted(("fam", gain), lay.elements[gain])), ("bb", 0, x[a:])]
            changes["gained"] = gain
    rel = Layout(out, lay.units, lay.elements)
    rel.changes = changes
    return rel


def put_n_at_repeat(lay, st, inside=True, beside=True):
    """N runs (code 5) at a repeat copy of the layout, in place: one inside the longest family or duplication copy, one that
    ends where another copy starts.  Returns the (start, length) of the runs in the text."""
    runs, o, spans = [], 0, []
    for k, (kind, _, x) in enumerate(lay.pieces):
        if kind in ("fam", "dup") and len(x) >= 40:
            spans.append((len(x), k, o))
        o += len(x)
    spans.sort(reverse=True)
    if inside and spans:
        n, k, o = spans[0]
        ln = min(st.randint(1, 40), n // 4)
        a = n // 2 - ln // 2
        lay.pieces[k][2][a:a + ln] = 5
        runs.append((o + a, ln))
    if beside and len(spans) > 1:
        n, k, o = spans[1]
        prev = lay.pieces[k - 1][2] if k > 0 else np.zeros(0, np.uint8)
        ln = min(st.randint(1, 30), len(prev))
        if ln:
            prev[len(prev) - ln:] = 5
            runs.append((o - ln, ln))
    return runs


def translocate(h, st, lo=500, hi=2000):
    """One block of lo-hi symbols (scaled down for short texts) cut out and put back elsewhere."""
    if len(h) < 40:
        return h
    hi = min(hi, len(h) // 4)
    lo = min(lo, max(1, hi // 2))
    ln = st.randint(lo, hi)
    a = st.randint(0, len(h) - ln - 1)
    blk = h[a:a + ln].copy()
    h = np.concatenate([h[:a], h[a + ln:]])
    b = st.randint(0, len(h) - 1)
    return np.ascontiguousarray(np.concatenate([h[:b], blk, h[b:]]))


def relative(lay, st, d, n_runs=False, lo=None, hi=None):
    """The codes of a relative of a layout: relative_layout, N runs at repeat copies where asked, one translocated block;
    cut or padded with random symbols into lo..hi where a range is given."""
    r = relative_layout(lay, st, d)
    for k, p in enumerate(r.pieces):                               # (own arrays: N runs are written in place)
        r.pieces[k] = (p[0], p[1], p[2].copy())
    if n_runs:
        put_n_at_repeat(r, st)
    h = translocate(r.codes(), st)
    if hi is not None and len(h) > hi:
        h = h[:hi]
    if lo is not None and len(h) < lo:
        h = np.concatenate([h, _rnd(st, lo - len(h))])
    return np.ascontiguousarray(h)


def repeat_stats(g, k):
    """(share, multiplicity) over the two-strand text of g (g, then its reverse complement; no window spans the two): the
    share of the windows of k symbols without N whose k-mer occurs more than once, and the largest number of
    occurrences of one k-mer."""
    g = np.asarray(g, dtype=np.uint8)
    vals = []
    for s in (g, rc(g)):
        w = len(s) - k + 1
        if w <= 0:
            continue
        isn = np.concatenate(([0], np.cumsum(s > 3)))
        valid = (isn[k:] - isn[:-k]) == 0
        c = np.where(s > 3, 0, s).astype(np.uint64)
        v = np.zeros(w, dtype=np.uint64)
        for j in range(k):
            v |= c[j:j + w] << np.uint64(2 * j)
        vals.append(v[valid])
    if not vals or sum(len(v) for v in vals) == 0:
        return 0.0, 0
    v = np.concatenate(vals)
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    return float((cnt[inv] > 1).mean()), int(cnt.max())


# ---- the named sets: util.instantiation_set's names, genome counts and length ranges -----------------------------------
SET_RANGES = {"small": (8500, 10000), "split": (17000, 25000)}
BIG_LEN = {"mid": 140_000, "long": 2_200_000}
_SETS = {}
_INFO = {}


def _family_set(seed, n, lo, hi, with_n):
    """n structured genomes of lo..hi symbols: two families of four -- a genome, two relatives at 0.5-15 % divergence and an
    exact copy; a genome, a relative, its whole-genome reverse complement and another relative -- then strangers.  with_n:
    the first genome gets an N run inside its longest repeat copy (beside util._put_n_runs's runs)."""
    st = SG.Stream(seed)
    margin = (hi - lo) // 4
    seqs, roots = [], []
    for f in range((n + 3) // 4):
        lay = structured_layout(st, st.randint(lo + margin, hi - margin))
        for k, p in enumerate(lay.pieces):
            lay.pieces[k] = (p[0], p[1], p[2].copy())
        g = lay.codes()
        div = lambda: 0.005 + 0.145 * st.one()
        if f == 0:
            fam = [g, relative(lay, st, div(), lo=lo, hi=hi), relative(lay, st, div(), lo=lo, hi=hi), g.copy()]
        elif f == 1:
            fam = [g, relative(lay, st, div(), lo=lo, hi=hi), rc(g), relative(lay, st, div(), lo=lo, hi=hi)]
        else:
            fam = [g]
        roots.append((len(seqs), lay))
        seqs += fam
    seqs = seqs[:n]
    info = {}
    if with_n:
        seqs = U._put_n_runs(seqs)
        idx, lay = roots[0]
        a, b = max(lay.spans(), key=lambda s: s[1] - s[0])
        mid = (a + b) // 2
        seqs[idx][mid:mid + 25] = 5
        info["n_in_repeat"] = (idx, mid, 25, (a, b))
    return [np.ascontiguousarray(s) for s in seqs], info


def repeat_set(name):
    """The repeat-structured counterpart of util.instantiation_set(name): the same names ('small', 'split', 'mid', 'long',
    each with ' N'), genome counts and length ranges -- small: 9 of 8.5-10 kbp; split: 8 of 17-25 kbp; mid: + one of
    140 kbp and a relative; long: + one of 2.2 Mbp and a relative -- and the genome of 300 bp last."""
    if name not in _SETS:
        base, with_n = name.split(" ")[0], name.endswith(" N")
        st = SG.Stream(4243)
        short = structured(st, 300)
        if base == "split":
            seqs, info = _family_set(4311, 8, *SET_RANGES["split"], with_n)
        else:
            seqs, info = _family_set(4312, 9, *SET_RANGES["small"], with_n)
        if base in BIG_LEN:
            L = BIG_LEN[base]
            lay = structured_layout(st, L)
            big = lay.codes()
            rel = relative(lay, st, 0.02)
            if with_n:
                big = big.copy()
                big[L // 3:L // 3 + 100] = 5
            seqs = [big, rel] + seqs[:8]
            if "n_in_repeat" in info:
                i, a, ln, span = info["n_in_repeat"]
                info["n_in_repeat"] = (i + 2, a, ln, span)
        _SETS[name] = [np.ascontiguousarray(s) for s in seqs] + [short]
        _INFO[name] = info
    return _SETS[name]


def repeat_set_info(name):
    repeat_set(name)
    return _INFO[name]


SET_NAMES = tuple(b + s for b in ("small", "split", "mid", "long") for s in ("", " N"))


def related_pairs(name):
    """(r, q) of the related pairs of a named set, both directions."""
    base = name.split(" ")[0]
    off = 2 if base in BIG_LEN else 0
    n_fam = 8 if base != "small" else 9
    fams = [[0, 1]] if off else []
    members = [k + off for k in range(8 if off else n_fam)]
    fams += [[m for m in members if (m - off) // 4 == f] for f in range(3)]
    return [(a, b) for fam in fams for a in fam for b in fam if a != b]


def checksum(seqs):
    c = 0
    for s in seqs:
        c = zlib.crc32(np.ascontiguousarray(s).tobytes(), zlib.crc32(len(s).to_bytes(8, "little"), c))
    return c


# ---- the exit sets: pairs laid out for single exits of the pair kernel's hand-written loops ------------------------------
# (tests/path_cover.py: the slots the random and the repeat-structured sets leave at zero)
EXIT_LEN, EXIT_STEP, EXIT_FIRST = 9000, 420, 300
EXIT_SET_NAMES = ("exits", "exits N")
# A motif is the bursts of a relative behind its start s, as (from, to) offsets: every symbol of a burst is substituted, there
# are no indels (the diagonal holds), and what lies between two bursts stays exact.  Each opens with a burst of 50 -- longer
# than mqd: the scan loses track and comes back through the anchor queue, which then covers the steps behind the next
# event, so the null chain (not the light rounds of a stretch the scan has outrun) looks at them -- then 18 exact symbols
# (an anchor under both tuples: the event the chain starts from) and a burst of 10.
EXIT_MOTIFS = {
    "long seed": ((0, 50), (68, 78)),                      # ... then >= 130 exact symbols: the seed's match runs over 64 + msl
    "several": ((0, 50), (68, 78), (90, 100)),             # ... then 12 exact whose first 10 stand 30 further on as well (exit_pair plants them)
    "short seeds": ((0, 50), (68, 78), (90, 100), (113, 123)),   # ... then seeds of 12 and 13: below mal 15, no anchor at their step
}
# the end of the text, as offsets from the end: 18 exact, a burst, a seed of 12 that starts 62 before the end (inside the
# last 64 + msl symbols: the chain's bounds test hands it back), a burst, 40 exact to the end
EXIT_TAIL = ((-140, -90), (-72, -62), (-50, -40))


def exit_pair(st, L=EXIT_LEN):
    """(g, h): a random genome and its relative by bursts, motif after motif of EXIT_MOTIFS every EXIT_STEP symbols and
    EXIT_TAIL at the end -- the null chain's exits 'long seed' (sw[4]), 'several' (sw[2]) and 'text end' (sw[3]), and a seed
    handed back by the bounds test with no anchor at its step (find_event's LZ_PS(1))."""
    g = _rnd(st, L)
    kinds = list(EXIT_MOTIFS)
    starts = list(range(EXIT_FIRST, L - EXIT_STEP - 200, EXIT_STEP))
    for k, s in enumerate(starts):
        if kinds[k % len(kinds)] == "several":
            g[s + 108:s + 118] = g[s + 78:s + 88]
    h = g.copy()
    shift = (st.u64(L) % np.uint64(3)).astype(np.uint8) + 1
    spans = [(s + a, s + b) for k, s in enumerate(starts) for a, b in EXIT_MOTIFS[kinds[k % len(kinds)]]]
    spans += [(L + a, L + b) for a, b in EXIT_TAIL]
    for a, b in spans:
        h[a:b] = (h[a:b] + shift[a:b]) % 4
    return np.ascontiguousarray(g), np.ascontiguousarray(h)


def exit_strand_end(g, st, L=8600):
    """A stranger to g that holds, 3,000 symbols in, the reverse complement of g's first 30 symbols -- as a query its match
    ends where the reference text ends, past the last complete seed window, and the null chain hands back nothing -- and
    300 symbols on 30 symbols of g's middle: the next queued candidate, plain, which find_event's common call takes
    (LZ_PS(2))."""
    return np.ascontiguousarray(np.concatenate([_rnd(st, 3000), rc(g[:30]), _rnd(st, 300), g[5000:5030], _rnd(st, L - 3360)]))


_EXIT_SETS = {}


def exit_set(name):
    """'exits': exit_pair's two genomes, exit_strand_end's stranger and a relative of the first at 5 %; ' N': the relative
    with N runs at its start, in its middle and at its end (the others stay N-free: a pair with an N leaves the chain's
    seed event at its bounds test)."""
    if name not in _EXIT_SETS:
        st = SG.Stream(4320)
        g, h = exit_pair(st)
        x = exit_strand_end(g, st)
        m = SG.mutate(g, 0.05, st)
        if name.endswith(" N"):
            m[:9] = 5
            m[len(m) // 2:len(m) // 2 + 40] = 5
            m[-5:] = 5
        _EXIT_SETS[name] = [np.ascontiguousarray(s) for s in (g, h, x, m)]
    return _EXIT_SETS[name]


# ---- fuzz cases ----------------------------------------------------------------------------------------------------------
def fuzz_seqs(st, lo, hi):
    """Five genomes of lo..hi symbols: a structured genome, two relatives with a translocation (one with N runs at its
    repeat copies, half of the time), a structured stranger and an exact copy."""
    lay = structured_layout(st, st.randint(lo, hi))
    g = lay.codes()
    a = relative(lay, st, 0.005 + 0.12 * st.one())
    b = relative(lay, st, 0.02 + 0.2 * st.one(), n_runs=st.one() < 0.5)
    return [g, a, b, structured(st, st.randint(lo, hi)), g.copy()]


def fuzz_set(seed):
    """The seeded CPU fuzz set: five genomes of 8-40 kbp."""
    return fuzz_seqs(SG.Stream(9000 + seed), 8000, 40000)


def fuzz_medium(st):
    """fuzz_case_medium's parameters on five structured genomes of 8-40 kbp."""
    prm, _ = U.fuzz_case_medium(st)
    return prm, fuzz_seqs(st, 8000, 40000)


def fuzz_short(st):
    """fuzz_case's parameters (the wide tuples among them) on five structured genomes of 50-1,500 bp: families, arrays and
    hairpins scaled down with the length."""
    prm, _ = U.fuzz_case(st)
    return prm, fuzz_seqs(st, 50, 1500)


