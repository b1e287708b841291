// The device tokenizer's route, decided apart from its launches: which of the cell kernels of pg_tokenize.hip takes a block, from
// the shape of its layout and two environment switches, and the LDS bytes that kernel is launched with.  Plain C++17 with no HIP
// header, so that a CPU program can walk the decision (tests/tok_plan_main.cpp); tok_parse (pg_tokenize.hip) carries it out.
#pragma once

#include <cstddef>
#include <cstdlib>

// what a block's kernels may ask of LDS (the tables and the rows being put together)
constexpr size_t PG_TOK_LDS_MAX = 60 * 1024;
// k_tok_cells3 keeps a lane's column-table entries in registers for up to this many trips of 64 columns
constexpr int PG_TOK_NIT_MAX = 4;

// ---- the switches ---------------------------------------------------------------------------------------------------------------
// Named here and nowhere else; tok_parse reads them once per process.
struct PgTokSwitches {
    int parse = 0;                 // PG_TOK_PARSE: 1 the first form (k_tok_parse + k_nib_pack), 2 k_tok_cells for every layout (A/B, tests)
    bool cells_regs = true;        // PG_TOK_CELLS_REGS=0: k_tok_cells3 reads its column table per step, whatever the column count
};

inline PgTokSwitches pg_tok_switches() {
    PgTokSwitches s;
    if (const char *e = getenv("PG_TOK_PARSE")) {
        const int v = atoi(e);
        s.parse = v == 1 || v == 2 ? v : 0;
    }
    if (const char *e = getenv("PG_TOK_CELLS_REGS")) s.cells_regs = atoi(e) != 0;
    return s;
}

// ---- the route ------------------------------------------------------------------------------------------------------------------
enum PgTokRoute {
    PG_TOK_ROUTE_PARSE = 0,        // k_tok_parse + k_nib_pack: a wavefront per line, tables in global memory
    PG_TOK_ROUTE_CELLS = 1,        // k_tok_heads + k_tok_cells: cells of any width
    PG_TOK_ROUTE_CELLS3 = 2,       // k_tok_heads + k_tok_cells3<FMT, nit>: every cell of at most three characters
};

struct PgTokPlan {
    PgTokRoute route;
    int nit;                       // CELLS3: the NIT the kernel is instantiated with (0: the table read per step); else 0
    size_t lds_bytes;              // dynamic LDS of the cell kernel's launch (PARSE: none)
};

// k_tok_cells: col_slot [n_cols][max_ploidy] | col_ploidy | col_off | col_w, then four rows of S bytes
inline size_t pg_tok_cells_lds(int n_cols, int max_ploidy, int S) { return (size_t)n_cols * (max_ploidy + 3) * 4 + 4 * (size_t)S; }
// k_tok_cells3: a packed table entry of 16 bytes per column, the diplo table, then four rows of S bytes + 64 dump bytes
inline size_t pg_tok_cells3_lds(int n_cols, int S) { return (size_t)n_cols * 16 + 256 + 4 * ((size_t)S + 64); }

// n_cols file columns (wanted or not), max_ploidy of the layout, S slots per row (a multiple of 16), widest: the widest cell of the
// block's first line in characters, wanted or not
inline PgTokPlan pg_plan_tok(int n_cols, int max_ploidy, int S, int widest, const PgTokSwitches &sw) {
    const size_t lds_bytes = pg_tok_cells_lds(n_cols, max_ploidy, S);
    if (lds_bytes > PG_TOK_LDS_MAX || sw.parse == 1) return {PG_TOK_ROUTE_PARSE, 0, 0};
    const size_t lds3 = pg_tok_cells3_lds(n_cols, S);
    if (widest > 3 || lds3 > PG_TOK_LDS_MAX || sw.parse == 2) return {PG_TOK_ROUTE_CELLS, 0, lds_bytes};
    const int nit = (n_cols + 63) / 64;
    return {PG_TOK_ROUTE_CELLS3, !sw.cells_regs || nit > PG_TOK_NIT_MAX ? 0 : nit, lds3};
}
