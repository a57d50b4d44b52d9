/* esdf_oracle_check.c -- oracle/backend_oracle.c: be_update_esdf2d under the address and undefined-behaviour sanitizers
 * (tests/test_esdf_cases_cpu.py compiles both files into one stand-alone program and runs it as a child process).
 *   usage: esdf_oracle_check <file>
 *   file:  one geometry per line: name nx ny res x_lo y_lo odom_x odom_y range
 *   out:   "<name> <state> rc written" for the all-free (1) and the all-occupied (2) grid of every geometry; written: the cells
 *          of the field that no longer hold DBL_MAX
 * The state grid is malloc'ed at exactly nx ny bytes and the field at nx ny doubles: a read or write past either is reported. */
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/backend_oracle.h"

int main(int argc, char **argv)
{
    FILE *f;
    char name[64];
    int nx, ny, state;
    double res, x_lo, y_lo, ox, oy, range;
    if (argc != 2) return 2;
    f = fopen(argv[1], "r");
    if (!f) return 2;
    while (fscanf(f, "%63s %d %d %lf %lf %lf %lf %lf %lf", name, &nx, &ny, &res, &x_lo, &y_lo, &ox, &oy, &range) == 9) {
        const size_t n = (size_t)nx * ny;
        for (state = 1; state <= 2; ++state) {
            unsigned char *grid = malloc(n);
            double *dist = malloc(sizeof(double) * n);
            size_t i, written = 0;
            int rc;
            if (!grid || !dist) return 3;
            memset(grid, state, n);
            for (i = 0; i < n; ++i) dist[i] = DBL_MAX;
            rc = be_update_esdf2d(grid, nx, ny, res, x_lo, y_lo, ox, oy, range, dist);
            for (i = 0; i < n; ++i) written += dist[i] != DBL_MAX;
            printf("%s %d %d %zu\n", name, state, rc, written);
            free(grid);
            free(dist);
            if (rc != 0) return 4;
        }
    }
    fclose(f);
    return 0;
}
