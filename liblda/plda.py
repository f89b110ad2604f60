"""liblda/plda.py -- the reference's `PLDA` class (python/liblda/plda.py:4-51): the same
four one-line delegations, onto plda_amd.MPlda (HIP kernels on MI355X)."""
from plda_amd.libplda import MPlda


class PLDA(object):

    def __init__(self, device=0):
        self._instance = MPlda(device)

    def fit(self, x, y, iters=10):
        """Fit the model on background data x (nsamples, featdim), uint labels y
        (plda.py:9-10)."""
        return self._instance.fit(x, y, iters)

    def transform(self, x, y):
        """Transform vectors x with labels y into the PLDA space: {label: (n, vector)}
        (plda.py:12-23)."""
        return self._instance.transform(x, y)

    def norm(self, vectors, transformedvecs, numutts=0):
        """Estimate z-norm mean/std of the enrol models `transformedvecs` against the
        held-out `vectors` (plda.py:25-37)."""
        return self._instance.norm(vectors, transformedvecs, numutts)

    def score(self, target, xvec, yvec):
        """Score enrol model xvec=(n, vec) of id `target` against test yvec=(n, vec)
        (plda.py:39-51).  Returns a float."""
        return self._instance.score(target, xvec, yvec)

    # ---- batched extensions (what the reference's callers loop over in Python) ----
    def score_matrix(self, enrol, test, znorm=True, calibrate=False):
        """float32 [M, Nt] matrix of score(id_i, enrol_i, test_j) in one launch (calibrate=True: mapped with the stored
        calibration)."""
        return self._instance.score_matrix(enrol, test, znorm, calibrate)

    def score_trials(self, enrol, test, e_idx, t_idx, znorm=True, calibrate=False):
        return self._instance.score_trials(enrol, test, e_idx, t_idx, znorm, calibrate)

    def calibrate(self, enrol, test, test_speaker, prior=0.5, znorm=True, cohort=None, top_k=None):
        """Fit and store the linear calibration llr = a * score + b on the trials between two transform() results (enrol keys
        are the speakers, test_speaker names the speaker of each test entry); returns a plda_amd.calibration.Calibration."""
        return self._instance.calibrate(enrol, test, test_speaker, prior, znorm, cohort, top_k)

    def fuse(self, enrol, test, test_speaker, others, prior=0.5, znorm=True, cohort=None, top_k=None):
        """Fit the linear fusion of this model's trials matrix with the fp32 [M, Nt] matrices `others` of other systems
        (prior-weighted logistic regression); returns a plda_amd.fusion.Fusion (not stored, not saved)."""
        return self._instance.fuse(enrol, test, test_speaker, others, prior, znorm, cohort, top_k)

    def score_matrix_fused(self, enrol, test, others, fusion, znorm=True, cohort=None, top_k=None, quality=None):
        """float32 [M, Nt]: the fused value of `fusion` over this model's matrix and `others` (and, with `quality`, the
        side-information terms of a `calibrate_quality` result)."""
        return self._instance.score_matrix_fused(enrol, test, others, fusion, znorm, cohort, top_k, quality)

    def calibrate_quality(self, enrol, test, test_speaker, quality, others=(), prior=0.5, znorm=True, cohort=None, top_k=None):
        """Quality-aware calibration: the fusion of this model's score (and `others`) with side-information terms
        `quality` = ((op, enrol_values, test_values), ...), op one of "min" | "max" | "sum" | "absdiff" | "prod" of the
        row's and the column's quality (duration, embedding norm, cohort mean ...), formed on the device without ever
        holding their matrices; returns a plda_amd.fusion.QualityFusion (not stored, not saved)."""
        return self._instance.calibrate_quality(enrol, test, test_speaker, quality, others, prior, znorm, cohort, top_k)

    def min_dcf(self, enrol, test, test_speaker, points=((0.01, 1.0, 1.0),), znorm=True, cohort=None, top_k=None, calibrate=False):
        """The exact minimum detection cost of the trials between two transform() results at up to 8 operating points
        (prior, c_miss, c_fa); returns (one dict per point, info)."""
        return self._instance.min_dcf(enrol, test, test_speaker, points, znorm, cohort, top_k, calibrate)

    def min_cllr(self, enrol, test, test_speaker, znorm=True, cohort=None, top_k=None):
        """minCllr and the ROC convex hull of the trials between two transform() results; returns (result dict, a
        plda_amd.rocch.Pav holding the hull's vertices and the PAV llrs)."""
        return self._instance.min_cllr(enrol, test, test_speaker, znorm, cohort, top_k)

    def partition(self, enrol, test, test_speaker, key=None, znorm=True, cohort=None, top_k=None, calibrate=False):
        """The per-(condition bucket, class) score lists of the trials under a plda_amd.trialkey.TrialKey (None: every pair),
        on the device; returns a plda_amd.trialkey.Partition."""
        return self._instance.partition(enrol, test, test_speaker, key, znorm, cohort, top_k, calibrate)

    def evaluate(self, enrol, test, test_speaker, key=None, points=((0.01, 1.0, 1.0),), znorm=True, cohort=None, top_k=None,
                 calibrate=False, prior=0.5):
        """EER, minDCF, actual DCF, Cllr and minCllr per condition bucket of a trial key, pooled and equalised; returns
        {"buckets": {name: figures}, "pooled": figures, "equalised": means}."""
        return self._instance.evaluate(enrol, test, test_speaker, key, points, znorm, cohort, top_k, calibrate, prior)

    def calibrate_pav(self, enrol, test, test_speaker, znorm=True, cohort=None, top_k=None):
        """Fit and store the PAV (pool adjacent violators) map of those trials; returns the plda_amd.rocch.Pav."""
        return self._instance.calibrate_pav(enrol, test, test_speaker, znorm, cohort, top_k)

    def cohort_stats(self, side, cohort, top_k=None):
        """(mean, std) of the top_k largest cohort scores of every row of `side` (AS-norm statistics)."""
        return self._instance.cohort_stats(side, cohort, top_k)

    def score_matrix_asnorm(self, enrol, test, cohort, top_k=None, calibrate=False):
        """float32 [M, Nt] matrix, every trial normalised on both sides against the top_k closest cohort vectors."""
        return self._instance.score_matrix_asnorm(enrol, test, cohort, top_k, calibrate)

    def score_trials_asnorm(self, enrol, test, e_idx, t_idx, cohort, top_k=None, calibrate=False):
        return self._instance.score_trials_asnorm(enrol, test, e_idx, t_idx, cohort, top_k, calibrate)

    def top_n(self, enrol, test, n=10, per="test", znorm=True, cohort=None, top_k=None, calibrate=False):
        """(scores float32 [L, n], ids int64 [L, n]): the n best enrol models of every test entry (per="test") or the n best
        test entries of every enrol model (per="enrol"), best first; the trials matrix is never held."""
        return self._instance.top_n(enrol, test, n, per, znorm, cohort, top_k, calibrate)

    def adapt(self, x, weights=None, within_scale=0.3, between_scale=0.7, mean_diff_scale=1.0):
        """Unsupervised domain adaptation of the model to the unlabelled rows x (Kaldi's PldaUnsupervisedAdaptor restated,
        parity unpinned); returns a plda_amd.adaptation.Adaptation.  Clears the z-norm statistics and the stored calibration."""
        return self._instance.adapt(x, weights, within_scale, between_scale, mean_diff_scale)

    def blend(self, other, alpha, alpha_mean=None):
        """Interpolate this model's covariances (and mean) with those of `other` (a PLDA, an MPlda or a (mean, transform,
        psi) triple); clears the z-norm statistics and the stored calibration."""
        self._instance.blend(other, alpha, alpha_mean)
        return self

    def cluster(self, x, offsets, threshold=0.0, num_speakers=None, return_merges=False, target_energy=None, method="ahc", **spectral):
        """Cluster the segments of R recordings (diarisation): x [T, featdim] raw segment vectors, recording r owning rows
        offsets[r] .. offsets[r+1]; average-linkage merging while the best pair's average score is at least `threshold` and
        more than `num_speakers` clusters are left.  target_energy=t: every recording is scored in the PCA subspace of its own
        vectors (Kaldi's --target-energy).  Returns (labels, n_clusters[, merges]); plda_amd/diarize.py.
        method="spectral": spectral clustering with auto-tuned pruning, no threshold (keywords p, p_fractions, max_speakers,
        max_iters, return_info); returns (labels, n_clusters[, info])."""
        if method != "ahc" or spectral:
            return self._instance.cluster(x, offsets, threshold, num_speakers, return_merges, target_energy=target_energy, method=method,
                                          **spectral)
        if target_energy is None:
            return self._instance.cluster(x, offsets, threshold, num_speakers, return_merges)
        return self._instance.cluster(x, offsets, threshold, num_speakers, return_merges, target_energy=target_energy)

    def cluster_corpus(self, x, threshold=0.0, num_speakers=None, return_merges=False):
        """Cluster a whole unlabelled corpus x [N, featdim] (N up to 32768, one problem on the whole device) into
        pseudo-speakers; returns (labels, n_clusters[, merges]); plda_amd/diarize.py."""
        return self._instance.cluster_corpus(x, threshold, num_speakers, return_merges)

    def adapt_clustered(self, x, threshold=0.0, num_speakers=None, alpha=0.5, alpha_mean=None, min_cluster_size=2, iters=10):
        """Clustering-based domain adaptation: cluster_corpus(x), fit an in-domain model on the pseudo-labels of the clusters of
        at least min_cluster_size rows, blend it in; returns a plda_amd.adaptation.ClusteredAdaptation.  Clears the z-norm
        statistics and the stored calibration."""
        return self._instance.adapt_clustered(x, threshold, num_speakers, alpha, alpha_mean, min_cluster_size, iters)

    def score_dense(self, x, offsets, target_energy, return_info=False):
        """Every recording's segment pairs scored in the PCA subspace of its own segment vectors; a list of [N_r, N_r] float32
        blocks[, {"dims", "eigenvalues"}]; plda_amd/diarize.py."""
        return self._instance.score_dense(x, offsets, target_energy, return_info)

    def resegment(self, x, offsets, labels, **vbx):
        """VBx resegmentation of the segments of R recordings from initial labels (cluster()'s); plda_amd/diarize.py."""
        return self._instance.resegment(x, offsets, labels, **vbx)

    def diarize(self, x, offsets, threshold=0.0, num_speakers=None, target_energy=None, method="ahc", **vbx):
        """cluster, then resegment.  target_energy goes to the clustering only (VBx keeps working on the full model).  Returns
        (labels, n_clusters[, info]); with overlap= (a per-segment bool mask) or min_posterior= (labels, n_clusters, labels2),
        labels2 the second speaker of every segment where one is kept, -1 elsewhere.  method="spectral" (keywords p,
        p_fractions, max_speakers): the spectral clustering's labels start VBx."""
        if method != "ahc":
            return self._instance.diarize(x, offsets, threshold, num_speakers, target_energy=target_energy, method=method, **vbx)
        if target_energy is None:
            return self._instance.diarize(x, offsets, threshold, num_speakers, **vbx)
        return self._instance.diarize(x, offsets, threshold, num_speakers, target_energy=target_energy, **vbx)

    def der(self, ref, hyp, offsets, dur=None, return_map=False, jer=False):
        """Diarisation error rate of R recordings from per-segment reference and hypothesis labels (-1 = non-speech), under
        the optimal speaker mapping; plda_amd/der.py.  Returns a DerResult (counts, der, total[, map]); jer=True adds the
        Jaccard error rate and the per-speaker figures (jer, jer_counts, jer_map, speakers)."""
        return self._instance.der(ref, hyp, offsets, dur, return_map, jer)

    def der_timed(self, turns, seg_start, seg_dur, hyp, offsets, collar=0, uem=None, skip_overlap=False, return_map=False, hyp2=None,
                  jer=False):
        """Time-based DER (md-eval's definition on integer ticks): overlapped reference turns, a collar, UEM regions; hyp2: a
        second hypothesis speaker per segment, -1 = none; jer=True adds the Jaccard error rate and the per-speaker figures;
        plda_amd/der.py: der_timed.  Returns a DerResult."""
        return self._instance.der_timed(turns, seg_start, seg_dur, hyp, offsets, collar, uem, skip_overlap, return_map, hyp2, jer)

    def tune_threshold(self, x, offsets, ref, thresholds, dur=None, target_energy=None, **timed):
        """The clustering threshold of the lowest pooled DER on a development set: one clustering (behind the per-recording PCA
        when target_energy is given), one sweep of its merge record.  Returns (threshold, SweepResult); plda_amd/der.py.
        With turns=, seg_start=, seg_dur= (and collar=, uem=, skip_overlap=) and ref=None the sweep is the time-based one.
        metric="jer" picks the threshold of the lowest pooled Jaccard error rate instead (the default, "der", is unchanged)."""
        if target_energy is not None:
            timed["target_energy"] = target_energy
        return self._instance.tune_threshold(x, offsets, ref, thresholds, dur, **timed)

    def transform_array(self, xbar, num_examples=1):
        return self._instance.transform_array(xbar, num_examples)

    def fit_embedding(self, x, y=None, kind="lda", dim=None, len_in=0.0, len_out=None):
        """Estimate the embedding chain in front of the model (centre, length-normalise, LDA / whitening, re-centre,
        length-normalise) from raw extractor output on the device and attach it; returns the plda_amd.embed.EmbeddingChain.
        From then on fit / transform / norm / adapt / cluster / resegment / diarize take raw rows."""
        return self._instance.fit_embedding(x, y, kind, dim, len_in, len_out)

    def set_embedding(self, chain):
        """Attach a plda_amd.embed.EmbeddingChain (None: remove it)."""
        self._instance.set_embedding(chain)

    def embed(self, x):
        """The attached chain applied to rows x [R, Din] (fp32 or fp64) -> float64 [R, Dout]."""
        return self._instance.embed(x)

    def save(self, path):
        return self._instance.save(path)

    def load(self, path):
        return self._instance.load(path)

    def save_kaldi(self, path, binary=True):
        """Write the model in Kaldi's `Plda` file layout (plda_amd/kaldi_io.py)."""
        return self._instance.save_kaldi(path, binary)

    def load_kaldi(self, path):
        self._instance.load_kaldi(path)
        return self
