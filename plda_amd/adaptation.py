"""plda_amd/adaptation.py -- what `MPlda.adapt` / `MPlda.adapt_update` return (csrc/adapt.hip; include/plda_hip.h, "PLDA domain
adaptation").  Kaldi's PldaUnsupervisedAdaptor restated from the published algorithm: PARITY UNPINNED, like the rest of the
PLDA path."""
import numpy as np

# Kaldi's PldaUnsupervisedAdaptorConfig defaults (restated, unpinned)
WITHIN_SCALE = 0.3
BETWEEN_SCALE = 0.7
MEAN_DIFF_SCALE = 1.0


class Adaptation(object):
    """Result of one unsupervised adaptation of a PLDA model.

    eigenvalues  float64 [D], descending: the in-domain total covariance in the basis where the model's total covariance
                 is the identity (1 = the variance the model already explains)
    n_excess     how many of them exceed 1 (directions in which the data shows more variance than the model)
    tot_weight   total weight of the rows the statistics were taken from
    rows         number of those rows
    mean_shift   ||new mean - old mean||_2
    """
    __slots__ = ("eigenvalues", "n_excess", "tot_weight", "rows", "mean_shift")

    def __init__(self, eigenvalues, n_excess, tot_weight, rows, mean_shift):
        self.eigenvalues = np.asarray(eigenvalues, np.float64)
        self.n_excess = int(n_excess)
        self.tot_weight = float(tot_weight)
        self.rows = int(rows)
        self.mean_shift = float(mean_shift)

    def __repr__(self):
        return "Adaptation(rows=%d, tot_weight=%g, n_excess=%d of %d, mean_shift=%g)" % (
            self.rows, self.tot_weight, self.n_excess, self.eigenvalues.shape[0], self.mean_shift)


class ClusteredAdaptation(object):
    """Result of one clustering-based adaptation (MPlda.adapt_clustered; Garcia-Romero et al. 2014).

    labels         int32 [N]: the pseudo-speaker of every corpus row, as cluster_corpus numbers them
    n_clusters     how many clusters the corpus fell into
    rows_kept      the rows the in-domain model was fitted on (those of clusters of at least min_cluster_size members)
    clusters_kept  the clusters they belong to
    """
    __slots__ = ("labels", "n_clusters", "rows_kept", "clusters_kept")

    def __init__(self, labels, n_clusters, rows_kept, clusters_kept):
        self.labels = np.asarray(labels, np.int32)
        self.n_clusters = int(n_clusters)
        self.rows_kept = int(rows_kept)
        self.clusters_kept = int(clusters_kept)

    def __repr__(self):
        return "ClusteredAdaptation(rows_kept=%d of %d, clusters_kept=%d of %d)" % (
            self.rows_kept, self.labels.shape[0], self.clusters_kept, self.n_clusters)
