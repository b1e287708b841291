// The rounds of the mergeGeno.py drop-in planned in plain host code, apart from the launches (pg_merge_dev.hip) and from the host route
// (pg_merge.cpp), which both ask it.  Every input file keeps a block of lines resident; a round writes the sites up to a HORIZON and
// carries everything behind it to the next round.
//
//   the horizon   the smallest last consumable key among the files that may still bring lines: sites up to it are final (no file can
//                 bring a line at or below it later, the keys of a file increase).  When no such file is left: the end of the .fai
//   dense methods (sites no file holds are written too) walk the positions of the genome, so their round is cut: it stays inside one
//                 scaffold and covers at most `max_positions` positions.  The output has a budget of its own, apart from the
//                 resident input: positions * (bytes of a line no file adds to) <= the budget; the cells the files add come on top
//                 and are bounded by the resident text.  A dense round therefore ends at the horizon, at its scaffold's end, or
//                 after exactly max_positions positions -- never earlier
//   a round is never empty while a file has lines left: the file that sets the horizon has its whole block consumed (and is read
//                 further before the next round); a dense round covers a position at least
// tests/merge_plan_main.cpp draws random key lists and block sizes and checks these properties.
#pragma once
#include <stdint.h>

struct pgm_site {
    int32_t scaf;
    int64_t pos;
};
inline bool operator<(const pgm_site &a, const pgm_site &b) { return a.scaf < b.scaf || (a.scaf == b.scaf && a.pos < b.pos); }
inline bool operator==(const pgm_site &a, const pgm_site &b) { return a.scaf == b.scaf && a.pos == b.pos; }

// what the plan knows of a file: whether lines may still follow its resident block, and the block's last consumable key
struct pgm_file_state {
    int32_t open;        // 1: the input goes on behind the block and the file has not stopped
    int32_t has_lines;   // the block holds a consumable line
    pgm_site last;       // its last one
};

struct pgm_round {
    pgm_site from;       // the sites of the round lie behind `from` ...
    pgm_site horizon;    // ... and up to `horizon`
    int32_t stalled;     // an open file holds no consumable line: read it further first (nothing may be written)
    int32_t last;        // nothing is left behind this round
};

// the last site of the genome (scaffold -1: the .fai holds no scaffold)
inline pgm_site pgm_genome_end(const int64_t *fai_len, int32_t n_fai) {
    if (n_fai <= 0) return pgm_site{-1, 0};
    return pgm_site{n_fai - 1, fai_len[n_fai - 1] > 0 ? fai_len[n_fai - 1] : 0};
}

// positions a dense round may cover: the output budget in lines that no file adds to (one at least).  The budget is the output's own:
// the resident input does not come off it
inline int64_t pgm_max_positions(int64_t out_budget, int64_t fixed_bytes) {
    const int64_t n = fixed_bytes > 0 ? out_budget / fixed_bytes : out_budget;
    return n > 1 ? n : 1;
}

// The next round behind `prev` (the horizon of the round before; {0, 0} at the start)
inline pgm_round pgm_plan_round(const pgm_file_state *files, int n_files, const int64_t *fai_len, int32_t n_fai, pgm_site prev, bool dense,
                                int64_t max_positions) {
    pgm_round R;
    R.from = prev;
    R.stalled = 0;
    const pgm_site end = pgm_genome_end(fai_len, n_fai);
    pgm_site h = end;
    bool any_open = false;
    for (int f = 0; f < n_files; ++f) {
        if (!files[f].open) continue;
        any_open = true;
        if (!files[f].has_lines) { R.stalled = 1; continue; }
        if (files[f].last < h) h = files[f].last;
    }
    if (h < prev) h = prev;                                        // (an open file's keys lie behind prev; the end of an empty genome may not)
    if (dense && n_fai > 0) {
        // behind the last position of a scaffold the round begins with the next one
        while (R.from.scaf < h.scaf && R.from.pos >= fai_len[R.from.scaf]) R.from = pgm_site{R.from.scaf + 1, 0};
        if (R.from.scaf < h.scaf) h = pgm_site{R.from.scaf, fai_len[R.from.scaf]};
        if (h.pos - R.from.pos > max_positions) h.pos = R.from.pos + max_positions;
    }
    R.horizon = h;
    R.last = !any_open && h == end;
    return R;
}
