// p2s_lsap.h -- the rectangular linear sum assignment problem, as scipy.optimize.linear_sum_assignment solves it
// (scipy 1.15.3, rectangular_lsap.cpp: the shortest augmenting path algorithm of D. F. Crouse, "On implementing 2D
// rectangular assignment algorithms", IEEE Trans. Aerospace and Electronic Systems 52(4), 2016), restated for the host
// and the device for matrices of up to 32 x 32.  The same assignment as scipy's, ties included, because every decision
// is scipy's:
//   * a matrix with more rows than columns is solved transposed, and the answer is sorted by row;
//   * the columns still to scan start in descending order (remaining[it] = nc - it - 1), and a scanned column is replaced
//     by the last one of the list;
//   * a column is preferred when its path cost is strictly lower, or equal and the column is unassigned;
//   * the duals are updated from the scanned rows and columns only;
//   * a NaN or -inf entry is refused before anything is solved, an assignment of infinite cost is "infeasible".
// Every floating-point operation is a single addition, subtraction or comparison: nothing for a compiler to contract.
#ifndef P2S_LSAP_H
#define P2S_LSAP_H

#if defined(__HIPCC__)
#define P2S_LSAP_HD __host__ __device__
#else
#define P2S_LSAP_HD
#endif

#define P2S_LSAP_MAX 32
#define P2S_LSAP_OK 0
#define P2S_LSAP_INVALID 1        // scipy: ValueError('matrix contains invalid numeric entries')
#define P2S_LSAP_INFEASIBLE 2     // scipy: ValueError('cost matrix is infeasible')

struct P2sLsapWork {              // about 1.2 KB: one per solver, in LDS on the device
    double u[P2S_LSAP_MAX], v[P2S_LSAP_MAX], shortest[P2S_LSAP_MAX];
    int path[P2S_LSAP_MAX], col4row[P2S_LSAP_MAX], row4col[P2S_LSAP_MAX], remaining[P2S_LSAP_MAX];
    unsigned char SR[P2S_LSAP_MAX], SC[P2S_LSAP_MAX];
};

// cost [n_rows][n_cols] row-major, 1 <= n_rows, n_cols <= 32.  -> P2S_LSAP_*; on P2S_LSAP_OK row_ind and col_ind hold the
// min(n_rows, n_cols) assigned pairs in ascending row order, as linear_sum_assignment returns them.
P2S_LSAP_HD inline int p2s_lsap_solve(int n_rows, int n_cols, const double *cost, P2sLsapWork &w, int *row_ind, int *col_ind) {
    const double inf = __builtin_huge_val();
    const bool transpose = n_cols < n_rows;
    const int nr = transpose ? n_cols : n_rows, nc = transpose ? n_rows : n_cols;
    const int rs = transpose ? 1 : n_cols, cs = transpose ? n_cols : 1;        // the solver's (i, j) is cost[i * rs + j * cs]
    for (int i = 0; i < n_rows * n_cols; ++i)
        if (cost[i] != cost[i] || cost[i] == -inf) return P2S_LSAP_INVALID;
    for (int i = 0; i < nr; ++i) { w.u[i] = 0.0; w.col4row[i] = -1; }
    for (int j = 0; j < nc; ++j) { w.v[j] = 0.0; w.path[j] = -1; w.row4col[j] = -1; }
    for (int cur = 0; cur < nr; ++cur) {
        // the shortest augmenting path from row `cur`
        double min_val = 0.0;
        int n_remaining = nc;
        for (int it = 0; it < nc; ++it) w.remaining[it] = nc - it - 1;
        for (int i = 0; i < nr; ++i) w.SR[i] = 0;
        for (int j = 0; j < nc; ++j) { w.SC[j] = 0; w.shortest[j] = inf; }
        int sink = -1, i = cur;
        while (sink == -1) {
            int index = -1;
            double lowest = inf;
            w.SR[i] = 1;
            for (int it = 0; it < n_remaining; ++it) {
                const int j = w.remaining[it];
                const double r = min_val + cost[i * rs + j * cs] - w.u[i] - w.v[j];
                if (r < w.shortest[j]) { w.path[j] = i; w.shortest[j] = r; }
                if (w.shortest[j] < lowest || (w.shortest[j] == lowest && w.row4col[j] == -1)) { lowest = w.shortest[j]; index = it; }
            }
            min_val = lowest;
            if (min_val == inf) return P2S_LSAP_INFEASIBLE;
            const int j = w.remaining[index];
            if (w.row4col[j] == -1) sink = j;
            else i = w.row4col[j];
            w.SC[j] = 1;
            w.remaining[index] = w.remaining[--n_remaining];
        }
        // the duals
        w.u[cur] += min_val;
        for (int r = 0; r < nr; ++r)
            if (w.SR[r] && r != cur) w.u[r] += min_val - w.shortest[w.col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (w.SC[j]) w.v[j] -= min_val - w.shortest[j];
        // augment
        int j = sink;
        while (true) {
            const int r = w.path[j];
            w.row4col[j] = r;
            const int next = w.col4row[r];
            w.col4row[r] = j;
            j = next;
            if (r == cur) break;
        }
    }
    if (!transpose) {
        for (int i = 0; i < nr; ++i) { row_ind[i] = i; col_ind[i] = w.col4row[i]; }
    } else {                                                  // solver row i is column i of the matrix, assigned to its row
        int n = 0;                                            // col4row[i]; row4col is that map's inverse: in row order
        for (int r = 0; r < nc; ++r)
            if (w.row4col[r] != -1) { row_ind[n] = r; col_ind[n] = w.row4col[r]; ++n; }
    }
    return P2S_LSAP_OK;
}

#endif
