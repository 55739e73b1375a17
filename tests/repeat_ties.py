"""Tie cases: hand-built pairs of 9-12 kbp (tag words in use) that pin WHICH occurrence of a repeated k-mer the parse takes.

The rules (the reference's parser.cpp):
- long anchors (518-530, 589-601): every occurrence on the probe chain is tried and a strictly longer match replaces the best;
  occurrences lie on the chain in text order, so among equally long matches the smallest text position wins.  The text is the
  reference, 2 * mrd separators, its reverse complement: a forward-strand position is smaller than any of the other strand.
- close seeds (555-579): a longer match wins, an equal length goes to the strictly smaller |pos - ref_pred_pos|, and on equal
  distance the earlier position stays.
- anchor against seed (604 onward): when both exist the anchor is taken if (1 - 4^-la)^(2 (T + 1 - la)) >
  (1 - 4^-ls)^(lit + mrd + 1 - ls), T the text length, lit the literals since the last match.

A case is a dict: name, ref, qry, probe (a query position inside the match in question), col, want, other.  The check
(tests/test_repeats.py on the oracle, tests/test_gpu_repeats.py compares every region of the device with the oracle's): exactly
one region holds the query position `probe`, and
- col "ref_at": the reference position that region aligns with the query position `at` -- ref_start + (at - seq_start), the
  start of the occurrence taken whatever the backward extension added in front -- is `want`; the other copy would give `other`;
- col "ref_end": the region's ref_end is `want`.  A close seed extends a region and cannot start one, so which of two seeds
  was taken shows at the region's end: the query goes on with symbols that match nothing near either seed."""
import numpy as np

import synth_genomes as SG
import util as U
from repeat_genomes import WIDTH_UNITS, rc

A, C_, G, T = 0, 1, 2, 3
GT16 = np.array([G, T, G, G, T, T, G, T, T, G, G, T, G, T, T, T], np.uint8)       # a G/T word: no 7-mer of it occurs twice


def _rnd(st, n):
    return (st.u64(n) % np.uint64(4)).astype(np.uint8)


def anchor_beats_seed(la, ls, lit, T, mrd):
    """The arbitration of parser.cpp:614-617 in exact arithmetic (the powers differ by far more than a rounding)."""
    from fractions import Fraction
    anchor = (1 - Fraction(1, 4 ** la)) ** (2 * (T + 1 - la))
    close = (1 - Fraction(1, 4 ** ls)) ** (lit + mrd + 1 - ls)
    return anchor > close


def tie_cases():
    """The cases at the defaults (mal 11, msl 7, mrd 40, mqd 40, reg 35)."""
    p = U.full_params()
    st = SG.Stream(0x71E)
    cases = []

    def add(name, ref, qry, probe, col, want, other, at=None):
        ref, qry = (np.ascontiguousarray(x, dtype=np.uint8) for x in (ref, qry))
        assert 9000 <= len(ref) <= 12000 and 9000 <= len(qry) <= 12000 and want != other, name
        cases.append(dict(name=name, ref=ref, qry=qry, probe=int(probe), at=int(probe if at is None else at), col=col, want=int(want),
                          other=int(other)))

    def rc_pos(ref_len, a, n):
        """Where the reverse complement of ref[a:a + n] starts in the two-strand text."""
        return ref_len + 2 * p["mrd"] + (ref_len - a - n)

    # (a) two exact copies of an element E with different flanks, the query carries E between neutral flanks: both anchors
    # are |E| long, the smaller position wins.  The query has an A on both sides of E and the reference a C or a G, so that
    # neither they nor their complements (the other strand) lengthen a match.
    E = _rnd(st, 400)
    qa, qb = _rnd(st, 4800), _rnd(st, 4800)
    f1, f2, f3 = _rnd(st, 2500), _rnd(st, 3000), _rnd(st, 3700)
    qa[-1] = qb[0] = A
    f1[-1] = f2[-1] = f3[0] = C_
    f2[0] = G
    p1, p2 = len(f1), len(f1) + len(E) + len(f2)
    ref = np.concatenate([f1, E, f2, E, f3])
    add("a_equal_anchors_first_copy", ref, np.concatenate([qa, E, qb]), len(qa) + 5, "ref_at", p1, p2, at=len(qa))
    # (b) the query carries 30 symbols of the second copy's flank behind E: the longer match wins, the second copy
    add("b_longer_anchor_second_copy", ref, np.concatenate([qa, E, f3[:30], qb]), len(qa) + 5, "ref_at", p2, p1, at=len(qa))
    # (c) E once forward and once reverse-complemented, in both orders, and the query's E reverse-complemented: a position
    # of the forward half against one of the reverse-complement half.  The forward half comes first.
    ref = np.concatenate([f1, E, f2, rc(E), f3])
    add("c_forward_then_rc", ref, np.concatenate([qa, E, qb]), len(qa) + 5, "ref_at", p1, rc_pos(len(ref), p2, len(E)), at=len(qa))
    ref = np.concatenate([f1, rc(E), f2, E, f3])
    add("c_rc_then_forward", ref, np.concatenate([qa, E, qb]), len(qa) + 5, "ref_at", p2, rc_pos(len(ref), p1, len(E)), at=len(qa))
    add("c_rc_then_forward_rc_query", ref, np.concatenate([qa, rc(E), qb]), len(qa) + 5, "ref_at", p1, rc_pos(len(ref), p2, len(E)),
        at=len(qa))

    # (d), (e) close seeds.  After a shared stretch P the query has `lit` symbols of poly-C against the reference's poly-A,
    # then a seed of 8 symbols of G/T (msl <= 8 < mal: no anchor), then poly-C again.  The reference's poly-A holds the seed
    # at pred - d1 and at pred + d2, pred = end of P + lit.  Nothing else near can match.
    def seeds(name, d1, d2, first_wins):
        lit, ls = 14, 8
        P = _rnd(st, 300)
        P[-1] = G
        pre, post = _rnd(st, 4500), _rnd(st, 5200)
        qpre, qpost = _rnd(st, 4700), _rnd(st, 4800)
        win = np.full(lit + d2 + ls + 60, A, np.uint8)
        a1, a2 = lit - d1, lit + d2
        assert 0 <= a1 and a1 + ls < a2 and d2 < p["mrd"]
        win[a1:a1 + ls] = GT16[:ls]
        win[a2:a2 + ls] = GT16[:ls]
        ref = np.concatenate([pre, P, win, post])
        qry = np.concatenate([qpre, P, np.full(lit, C_, np.uint8), GT16[:ls], np.full(30, C_, np.uint8), qpost])
        base = len(pre) + len(P)
        ends = (base + a1 + ls, base + a2 + ls)
        add(name, ref, qry, len(qpre) + len(P) + lit + 2, "ref_end", ends[0 if first_wins else 1], ends[1 if first_wins else 0])

    seeds("d_equal_distance_earlier_seed", 6, 6, True)
    seeds("e_later_seed_is_nearer", 7, 6, False)
    seeds("e_earlier_seed_is_nearer", 6, 7, True)

    # (f) an anchor and a seed at one query position.  As (d), with one seed at the predicted place, and far away in the
    # reference the word W of la symbols whose first 8 are the seed, a mismatch, and 40 symbols Y the query carries too: when
    # the anchor is taken a region starts at W (and lives: W, a mismatch and Y make 54 symbols); when the seed is taken the
    # region of P ends with it.  la = 12 and 13 lie either side of the crossover at these lengths (anchor_beats_seed).
    def arb(name, la):
        lit, ls = 14, 8
        P = _rnd(st, 300)
        P[-1] = G
        W, Y = GT16[:la], _rnd(st, 40)
        Y[0] = Y[-1] = G
        pre, mid, post = _rnd(st, 3000), _rnd(st, 3000), _rnd(st, 3300)
        qpre, qpost = _rnd(st, 4700), _rnd(st, 4800)
        win = np.full(lit + ls + 60, A, np.uint8)
        win[lit:lit + ls] = W[:ls]
        far = np.concatenate([[A], W, [A], Y, np.full(20, A, np.uint8)]).astype(np.uint8)
        ref = np.concatenate([pre, P, win, mid, far, post])
        qry = np.concatenate([qpre, P, np.full(lit, C_, np.uint8), W, [C_], Y, np.full(20, C_, np.uint8), qpost]).astype(np.uint8)
        seed_end = len(pre) + len(P) + lit + ls
        anchor_pos = len(pre) + len(P) + len(win) + len(mid) + 1
        at = len(qpre) + len(P) + lit
        T = 2 * len(ref) + 3 * p["mrd"]
        if anchor_beats_seed(la, ls, lit, T, p["mrd"]):
            add(name, ref, qry, at + 2, "ref_at", anchor_pos, len(pre) + len(P) + lit, at=at)
        else:
            add(name, ref, qry, at + 2, "ref_end", seed_end, anchor_pos + la)

    arb("f_seed_beats_anchor_of_12", 12)
    arb("f_anchor_of_13_beats_seed", 13)

    # (g) a tandem array against itself shifted by every s = 1 .. unit - 1 symbols (the array at every offset inside a 16-symbol
    # tag word, a 32-symbol packed word and a 64-lane wave: 109 cases): the query's array starts s symbols into
    # the unit, so its first k-mer occurs in every unit of the reference's array; all those matches run to the end of the
    # query's array, which is two units shorter, so they are equally long and the first one is taken.
    for unit in WIDTH_UNITS:
        u = _rnd(st, unit)
        reps = 12
        arr = np.tile(u, reps)
        pre, post = _rnd(st, 4000), _rnd(st, 9500 - 4000 - len(arr))
        pre[-1] = (u[-1] + 1) % 4                                    # (the array does not start one symbol early)
        ref = np.concatenate([pre, arr, post])
        for s in range(1, unit):
            qpre, qpost = _rnd(st, 4400), _rnd(st, 4600)
            body = np.tile(u, reps + 1)[s:s + (reps - 2) * unit]
            # more than mqd symbols of N in front of the array: no chance match of the random flank reaches into it (a short
            # region that is dropped later would still have moved the scan past the array's start), the scan arrives out of
            # tracking mode and the match starts exactly at the array
            qpre[-45:] = 5
            add("g_tandem_unit%d_shift%d" % (unit, s), ref, np.concatenate([qpre, body, qpost]), len(qpre) + 5, "ref_at",
                len(pre) + s, len(pre) + s + unit, at=len(qpre))
    return cases


COLS = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")


def occurrence(case, regs):
    """What the regions of a pair (rows of COLS) say about the case: the value of its column, by the one region that holds
    the query position `probe`."""
    hold = [r for r in np.asarray(regs).tolist() if r[2] <= case["probe"] < r[3]]
    assert len(hold) == 1, (case["name"], hold)
    r = hold[0]
    return r[1] if case["col"] == "ref_end" else r[0] + (case["at"] - r[2])
