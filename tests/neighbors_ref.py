"""`dandd neighbors` restated in plain numpy: cardinalities in, the rows of its three files out (test infrastructure).

Nothing here is shared with dandd_amd: the window delta, the K-independent Jaccard, the ranking and the summary are
written out once more from what the issue says of them."""
import numpy as np

COLS = {
    "neighbors": ["sample", "fasta", "sample_delta", "sample_k", "genome_delta", "genome_k", "union_delta", "union_k", "KIJ", "rank"],
    "neighbors_summary": ["sample", "sample_delta", "sample_k", "best_fasta", "best_KIJ", "second_fasta", "second_KIJ", "collection_delta",
                          "with_sample_delta", "delta_added"],
    "neighbors_j": ["sample", "fasta", "kval", "Scard", "Gcard", "SGcard", "jaccard"],
}


def delta(cards, ks):
    """the largest card / k over the window, the larger k winning a tie -> (delta, k)"""
    ratio = np.asarray(cards, dtype=np.float64) / np.asarray(ks, dtype=np.float64)
    at = len(ks) - 1 - int(np.argmax(ratio[::-1]))
    return float(ratio[at]), int(ks[at])


def rows(samples, fastas, ks, scard, gcard, sgcard, ucard, uscard, top=None):
    """scard [ns][K] |S|, gcard [n][K] |G|, sgcard [ns][n][K] |S U G|, ucard [K] |all G|, uscard [ns][K] |all G U S|
    -> (neighbors, summary, j) rows as lists under COLS"""
    near, summary, jac = [], [], []
    du = delta(ucard, ks)[0]
    for s, sample in enumerate(samples):
        ds, ks_ = delta(scard[s], ks)
        cells = []
        for j, fasta in enumerate(fastas):
            dg, kg = delta(gcard[j], ks)
            dsg, ksg = delta(sgcard[s][j], ks)
            cells.append((-((ds + dg - dsg) / dsg), j, fasta, dg, kg, dsg, ksg))
        cells.sort(key=lambda c: (c[0], c[1]))                  # KIJ descending, then the universe's order
        for rank, (neg, _, fasta, dg, kg, dsg, ksg) in enumerate(cells[:top], 1):
            near.append([sample, fasta, ds, ks_, dg, kg, dsg, ksg, -neg, rank])
        second = (cells[1][2], -cells[1][0]) if len(cells) > 1 else (None, None)
        dus = delta(uscard[s], ks)[0]
        summary.append([sample, ds, ks_, cells[0][2], -cells[0][0], second[0], second[1], du, dus, dus - du])
        for j, fasta in enumerate(fastas):
            for kk, k in enumerate(ks):
                a, b, ab = float(scard[s][kk]), float(gcard[j][kk]), float(sgcard[s][j][kk])
                jac.append([sample, fasta, int(k), a, b, ab, (a + b - ab) / ab])
    return near, summary, jac
