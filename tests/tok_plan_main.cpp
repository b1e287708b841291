// csrc/pg_tok_plan.h walked as a program of its own (no GPU, no library): the route of the device tokenizer for the shapes given on
// the command line, under the switches of the environment (PG_TOK_PARSE, PG_TOK_CELLS_REGS -- read through pg_tok_switches, as
// tok_parse reads them).
//   tok_plan_main N_COLS:MAX_PLOIDY:S:WIDEST ...
// prints one line per shape:   N_COLS MAX_PLOIDY S WIDEST ROUTE NIT LDS_BYTES      (ROUTE: PARSE, CELLS or CELLS3)
// and checks what every plan must hold whatever the shape: a launch within the LDS limit, NIT == ceil(N_COLS / 64) <= 4 or 0, cells
// wider than three characters never in k_tok_cells3.  Exit status 1 on a bad argument or a plan that breaks these.
#include "../genomics_general_amd/csrc/pg_tok_plan.h"

#include <cstdio>

int main(int argc, char **argv) {
    const PgTokSwitches sw = pg_tok_switches();
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        int n_cols = 0, max_ploidy = 0, S = 0, widest = 0;
        char tail = 0;
        if (sscanf(argv[a], "%d:%d:%d:%d%c", &n_cols, &max_ploidy, &S, &widest, &tail) != 4 || n_cols < 1 || max_ploidy < 1 || S < 16 || S % 16 ||
            widest < 1) {
            fprintf(stderr, "tok_plan_main: bad shape '%s' (N_COLS:MAX_PLOIDY:S:WIDEST, S a multiple of 16)\n", argv[a]);
            return 1;
        }
        const PgTokPlan p = pg_plan_tok(n_cols, max_ploidy, S, widest, sw);
        const char *name = p.route == PG_TOK_ROUTE_PARSE ? "PARSE" : p.route == PG_TOK_ROUTE_CELLS ? "CELLS" : "CELLS3";
        printf("%d %d %d %d %s %d %zu\n", n_cols, max_ploidy, S, widest, name, p.nit, p.lds_bytes);
        const int nit = (n_cols + 63) / 64;
        bool ok = p.lds_bytes <= PG_TOK_LDS_MAX;
        if (p.route == PG_TOK_ROUTE_PARSE) ok = ok && p.nit == 0 && p.lds_bytes == 0;
        if (p.route == PG_TOK_ROUTE_CELLS) ok = ok && p.nit == 0 && p.lds_bytes == pg_tok_cells_lds(n_cols, max_ploidy, S);
        if (p.route == PG_TOK_ROUTE_CELLS3)
            ok = ok && widest <= 3 && sw.parse == 0 && p.lds_bytes == pg_tok_cells3_lds(n_cols, S) &&
                 (p.nit == 0 ? (!sw.cells_regs || nit > PG_TOK_NIT_MAX) : (sw.cells_regs && p.nit == nit && nit <= PG_TOK_NIT_MAX));
        if (sw.parse == 1) ok = ok && p.route == PG_TOK_ROUTE_PARSE;
        if (!ok) {
            fprintf(stderr, "tok_plan_main: the plan of '%s' breaks its rules\n", argv[a]);
            ++bad;
        }
    }
    return bad ? 1 : 0;
}
