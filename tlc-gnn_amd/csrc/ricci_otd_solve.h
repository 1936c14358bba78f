// ricci_otd_solve.h -- the exact integer transportation solver of ricci_otd.hip, free of HIP so that a host harness can compile
// it (tests/aids/otd_solve_host.cpp: OTD_DEV inline, Sync a no-op or a thread barrier) and compare it with an LP.
//
// Problem: sources i < na with integer excess exA[i], sinks j < nb with integer deficit exB[j] (equal totals), cost of a unit on
// (i, j) = the 2-bit hop code c(i, j) in {0, 1, 2, 3}.  Primal-dual (Ford-Fulkerson's transportation method) with integer
// potentials: arcs with reduced cost r = c - potA[i] - potB[j] == 0 are admissible, forward from a source, backward over an arc
// that carries flow.  A round is one level-synchronous search of the admissible residual graph from every source with excess,
// every step one sweep of the whole matrix by all threads, followed by the pushes along the search tree to every reached sink
// that still has a deficit (one thread; the paths are a few arcs long).  A round that reaches no deficit raises the potentials of
// the reached sources and lowers those of the reached sinks by delta = the least reduced cost leaving the reached set.
//
// Let L be the sum of the deltas so far.  Every source with excess has been raised every time and no sink with a deficit ever
// lowered, so every augmenting path costs exactly L a unit, and L <= c(i, j) <= 3 for any such pair: at most three potential
// changes, and once L is 3 all that is left moves at 3 a unit, without a search.  W = sum over pushes of amount * L.
//
// Bounds: a search has at most na + nb steps (a step that reaches nothing ends it), a path at most na + nb arcs, and the rounds
// are capped at 4 * (na + nb) + 64: every round pushes along at least one shortest path or changes the potentials (three times
// at most), and every push exhausts an excess, a deficit or the flow of an arc.  The proven cap for shortest-path pushes is
// Edmonds-Karp's V * E / 2 per level, useless as a watchdog; the cap here is four times the most rounds a naive one-push-per-search
// solver was seen to need.  A solve that exhausts it returns -1: the caller reports NaN, never a wrong value.
#ifndef TLC_RICCI_OTD_SOLVE_H
#define TLC_RICCI_OTD_SOLVE_H

#ifndef OTD_DEV
#define OTD_DEV __device__ __forceinline__
#endif

namespace otd {

enum : unsigned char { UNREACHED = 0, DONE = 1, FRONT = 2, NEXT = 3 };
enum : unsigned short { ROOT = 0xffffu };
enum { SH_ANY = 0, SH_F = 1, SH_B = 2, SH_PUSHED = 3, SH_DELTA = 4, SH_FAIL = 5, SH_INTS = 8 };      // the control block (ints of LDS)
constexpr int NO_DELTA = 1 << 20;

// (code_at of ricci_codes.h again: this header has to compile without HIP, that one cannot)
OTD_DEV int code_of(const unsigned int* codes, int q) { return (int)((codes[q >> 4] >> ((q & 15) * 2)) & 3u); }

OTD_DEV int round_cap(int na, int nb) { return 4 * (na + nb) + 64; }

// The cells q = tid, tid + W, ... of the na x nb matrix as (i, j) without a division per cell.
template <int W>
struct CellWalk {
    int i, j, q, di, dj, nb, cells;
    OTD_DEV CellWalk(int na, int nb_, int tid) : nb(nb_), cells(na * nb_) { q = tid; i = tid / nb_; j = tid - i * nb_; di = W / nb_; dj = W - di * nb_; }
    OTD_DEV bool ok() const { return q < cells; }
    OTD_DEV void next() { q += W; i += di; j += dj; if (j >= nb) { j -= nb; ++i; } }
};

// Cell: unsigned type of one flow cell (holds min(excess, deficit) of any pair); Ex: signed type of the excesses and of W.
// x: na * nb cells; stA / potA / parA: na entries, stB / potB / parB: nb entries; sh: SH_INTS ints.  All threads of the group call
// it; Sync()() is the group barrier.  Returns W on thread 0 (other threads: unspecified), -1 on every thread when a bound ran out.
// rounds_out (the host test's; the kernels pass none): the rounds used, to be held against round_cap(na, nb).
template <int W, class Cell, class Ex, class Sync, class AtomicMin>
OTD_DEV long long solve(const unsigned int* codes, int na, int nb, Cell* x, Ex* exA, Ex* exB, unsigned short* parA, unsigned short* parB,
                        unsigned char* stA, unsigned char* stB, signed char* potA, signed char* potB, int* sh, int tid, Sync sync,
                        AtomicMin atomic_min, int* rounds_out = nullptr) {
    const int cells = na * nb;
    for (int q = tid; q < cells; q += W) x[q] = 0;
    for (int i = tid; i < na; i += W) potA[i] = 0;
    for (int j = tid; j < nb; j += W) potB[j] = 0;
    if (tid == 0) { sh[SH_ANY] = 0; sh[SH_F] = 0; sh[SH_B] = 0; sh[SH_FAIL] = 0; }
    sync();
    long long cost = 0;                                   // thread 0's
    int level = 0;                                        // L, the same on every thread
    const int max_rounds = round_cap(na, nb);
    const int max_steps = na + nb + 1;
    int round = 0;
    for (; round < max_rounds; ++round) {
        for (int i = tid; i < na; i += W) {
            const bool root = exA[i] > 0;
            stA[i] = root ? FRONT : UNREACHED;
            parA[i] = ROOT;
            if (root) sh[SH_ANY] = 1;
        }
        for (int j = tid; j < nb; j += W) stB[j] = UNREACHED;
        sync();
        if (!sh[SH_ANY]) break;                           // nothing left to move: done
        int step = 0;
        for (; step < max_steps; ++step) {
            // forward: an unreached sink next to a frontier source over an admissible arc
            for (CellWalk<W> c(na, nb, tid); c.ok(); c.next()) {
                if (stA[c.i] == FRONT && stB[c.j] == UNREACHED && code_of(codes, c.q) - potA[c.i] - potB[c.j] == 0) {
                    parB[c.j] = (unsigned short)c.i;      // several sources may race: any of them is a parent at this depth
                    stB[c.j] = NEXT;
                    sh[SH_F] = 1;
                }
            }
            sync();
            for (int i = tid; i < na; i += W) if (stA[i] == FRONT) stA[i] = DONE;
            for (int j = tid; j < nb; j += W) if (stB[j] == NEXT) stB[j] = FRONT;
            const int f = sh[SH_F];
            if (tid == 0) sh[SH_B] = 0;
            sync();
            if (!f) break;
            // backward: an unreached source that sends flow to a frontier sink
            for (CellWalk<W> c(na, nb, tid); c.ok(); c.next()) {
                if (stB[c.j] == FRONT && stA[c.i] == UNREACHED && x[c.q] > 0) {
                    parA[c.i] = (unsigned short)c.j;
                    stA[c.i] = NEXT;
                    sh[SH_B] = 1;
                }
            }
            sync();
            for (int j = tid; j < nb; j += W) if (stB[j] == FRONT) stB[j] = DONE;
            for (int i = tid; i < na; i += W) if (stA[i] == NEXT) stA[i] = FRONT;
            const int b = sh[SH_B];
            if (tid == 0) sh[SH_F] = 0;
            sync();
            if (!b) break;
        }
        if (step >= max_steps) { if (tid == 0) sh[SH_FAIL] = 1; }       // cannot happen: every step reaches a new node
        // pushes along the tree, to every reached sink with a deficit
        if (tid == 0) {
            int pushed = 0;
            for (int j = 0; j < nb; ++j) {
                if (exB[j] <= 0 || stB[j] == UNREACHED) continue;
                Ex bott = exB[j];
                int cj = j, len = 0;
                bool ok = true;
                for (;;) {
                    const int i = parB[cj];
                    const int pj = parA[i];
                    if (pj == ROOT) { if (exA[i] < bott) bott = exA[i]; break; }
                    const Ex back = (Ex)x[i * nb + pj];
                    if (back < bott) bott = back;
                    cj = pj;
                    if (++len > na + nb) { ok = false; break; }
                }
                if (!ok) { sh[SH_FAIL] = 1; break; }
                if (bott <= 0) continue;
                cj = j;
                for (;;) {
                    const int i = parB[cj];
                    x[i * nb + cj] = (Cell)(x[i * nb + cj] + (Cell)bott);
                    const int pj = parA[i];
                    if (pj == ROOT) { exA[i] -= bott; break; }
                    x[i * nb + pj] = (Cell)(x[i * nb + pj] - (Cell)bott);
                    cj = pj;
                }
                exB[j] -= bott;
                cost += (long long)bott * level;
                pushed = 1;
            }
            sh[SH_PUSHED] = pushed;
            sh[SH_DELTA] = NO_DELTA;
            sh[SH_ANY] = 0;
            sh[SH_F] = 0;
        }
        sync();
        if (sh[SH_FAIL]) return -1;
        if (sh[SH_PUSHED]) continue;
        // no deficit within reach: delta = least reduced cost from a reached source to an unreached sink
        int dmin = NO_DELTA;
        for (CellWalk<W> c(na, nb, tid); c.ok(); c.next()) {
            if (stA[c.i] != UNREACHED && stB[c.j] == UNREACHED) {
                const int r = code_of(codes, c.q) - potA[c.i] - potB[c.j];
                if (r < dmin) dmin = r;
            }
        }
        if (dmin < NO_DELTA) atomic_min(&sh[SH_DELTA], dmin);
        sync();
        const int delta = sh[SH_DELTA];
        if (delta <= 0 || delta >= NO_DELTA) return -1;   // an unbalanced problem or a broken invariant
        level += delta;
        if (level >= 3) {                                 // every remaining (excess, deficit) pair is three hops apart
            if (level > 3) return -1;
            if (tid == 0) {
                for (int i = 0; i < na; ++i) cost += 3ll * (long long)exA[i];
                if (rounds_out) *rounds_out = round + 1;
            }
            return cost;
        }
        for (int i = tid; i < na; i += W) if (stA[i] != UNREACHED) potA[i] = (signed char)(potA[i] + delta);
        for (int j = tid; j < nb; j += W) if (stB[j] != UNREACHED) potB[j] = (signed char)(potB[j] - delta);
        sync();
    }
    if (round >= max_rounds) return -1;
    if (tid == 0 && rounds_out) *rounds_out = round;
    return cost;
}

}  // namespace otd
#endif
