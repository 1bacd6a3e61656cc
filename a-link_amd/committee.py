"""committee — drop-in for reference code/committee.py.

Bagging.predict (code/committee.py:13-20) = sum of member predictions / number of members.  When every
member is a device-resident DenseHead the mean is fused on the GPU (alink_committee_forward: member
softmaxes accumulated in member order, one divide); any other duck-typed member falls back to the
reference's own host arithmetic on the members' outputs.
attackModel / resize (code/committee.py:22-37) drive the noise objects (noise.py) and resize with
the device bilinear kernel (cv2.resize INTER_LINEAR rule, alink_resize_bilinear).
"""
import numpy as np

from . import head as _head


class Bagging:
    def __init__(self, models, attacks):
        self.models = models
        self.attacks = []
        for attack in attacks:
            self.attacks.append(attack)

    def _device_heads(self):
        hs = [getattr(m, "siamese_net", None) for m in self.models]
        if all(isinstance(h, _head.DenseHead) for h in hs) and \
                all(getattr(m, "_identity_preprocess", False) for m in self.models):
            return hs
        return None

    def predict(self, predict_on):
        hs = self._device_heads()
        if hs is not None:
            out = _head.committee_predict_device(hs, predict_on[0], predict_on[1])
            return out if isinstance(predict_on[0], hs[0].torch.Tensor) else out.cpu().numpy()
        predictions = []
        for model in self.models:
            predictions.append(model.predict(predict_on))
        predicted = np.sum(np.array(predictions), axis=0) / len(self.models)
        return np.array(predicted)

    def predict_indexed(self, emb_left, emb_right, li, ri):
        """Extension: score pairs (li[p], ri[p]) gathered from embedding matrices on device.  emb_left /
        emb_right may be lists with one matrix per member (each member behind its own feature extractor)."""
        hs = self._device_heads()
        if hs is None:
            raise TypeError("predict_indexed needs DenseHead members")
        return _head.committee_predict_device(hs, emb_left, emb_right, li, ri)

    def disagreement(self, predict_on, kind="vote_entropy"):
        """Extension: how far the members DISAGREE on every pair of predict_on = [left, right] — `kind` is vote_entropy,
        consensus_entropy or max_disagreement (disagreement.py; modAL.disagreement's measures), which predict's mean cannot
        give.  DenseHead members: the members' probabilities and the measure stay on the GPU (one launch for the measure);
        any other duck-typed member: the host formulas on the members' predict outputs."""
        from . import disagreement as _dis
        if kind not in _dis.KINDS:
            raise ValueError("unknown disagreement kind %r: choose among %s" % (kind, list(_dis.KINDS)))
        hs = self._device_heads()
        if hs is not None:
            probs = _head.committee_member_probs_device(hs, predict_on[0], predict_on[1])
            out = _dis.score_members_device(probs, want=(kind,))[kind]
            return out if isinstance(predict_on[0], hs[0].torch.Tensor) else out.cpu().numpy()
        proba = np.stack([np.asarray(model.predict(predict_on)) for model in self.models], axis=1)       # (P, M, C)
        if proba.ndim != 3 or proba.shape[2] < 2:
            raise TypeError("committee disagreement needs class probabilities: a one-column member has no vote to count")
        if kind == "vote_entropy":
            return _dis.votes_entropy(np.argmax(proba, axis=2), range(proba.shape[2]))
        return _dis.proba_consensus_entropy(proba) if kind == "consensus_entropy" else _dis.proba_max_disagreement(proba)

    def disagreement_indexed(self, emb_left, emb_right, li, ri, kind="vote_entropy"):
        """Extension: disagreement over pairs (li[p], ri[p]) gathered from embedding matrices on device, as predict_indexed."""
        from . import disagreement as _dis
        if kind not in _dis.KINDS:
            raise ValueError("unknown disagreement kind %r: choose among %s" % (kind, list(_dis.KINDS)))
        hs = self._device_heads()
        if hs is None:
            raise TypeError("disagreement_indexed needs DenseHead members")
        probs = _head.committee_member_probs_device(hs, emb_left, emb_right, li, ri)
        return _dis.score_members_device(probs, want=(kind,))[kind]

    def egl_indexed(self, emb_left, emb_right, li, ri):
        """Extension: the committee's expected gradient length (egl.py) of the pairs (li[p], ri[p]) gathered from embedding
        matrices on device — the mean over the members of each member's OWN EGL (a member's gradient is its own), summed in
        member order on the device, one divide.  emb_left / emb_right may be lists with one matrix per member, as in
        predict_indexed.  -> (P,) float32 on the device."""
        from . import egl as _egl
        hs = self._device_heads()
        if hs is None:
            raise TypeError("egl_indexed needs DenseHead members")
        per_member = isinstance(emb_left, (list, tuple))
        if per_member and (len(emb_left) != len(hs) or not isinstance(emb_right, (list, tuple)) or len(emb_right) != len(hs)):
            raise ValueError("%d members but %d / %d feature matrices" % (len(hs), len(emb_left), len(emb_right) if isinstance(emb_right, (list, tuple)) else 1))
        out = None
        for m, h in enumerate(hs):
            L, R = (emb_left[m], emb_right[m]) if per_member else (emb_left, emb_right)
            out = _egl.expected_gradient_length_device(h, L, R, li, ri, egl_out=out, accumulate=m > 0,
                                                       final_div=float(len(hs)) if m == len(hs) - 1 else 0.0)["egl"]
        return out

    def badge_indexed(self, emb_left, emb_right, li, ri, n_instances, uniforms=None, seed=None):
        """Extension: a BADGE batch (badge.py) of the pairs (li[p], ri[p]) gathered from embedding matrices on device.  The
        committee's gradient embedding of a pair is its members' embeddings side by side (a member's gradient is its own):
        D = members x out_dim x h2 columns, at most the 8,192 a picked row may have; k-means++ seeding over those rows.
        emb_left / emb_right may be lists with one matrix per member, as in egl_indexed.
        -> (idx int32 (k,), potential float64 (k,)) on the device, badge.kmeans_pp_device's."""
        from . import badge as _badge, egl as _egl
        hs = self._device_heads()
        if hs is None:
            raise TypeError("badge_indexed needs DenseHead members")
        per_member = isinstance(emb_left, (list, tuple))
        if per_member and (len(emb_left) != len(hs) or not isinstance(emb_right, (list, tuple)) or len(emb_right) != len(hs)):
            raise ValueError("%d members but %d / %d feature matrices" % (len(hs), len(emb_left), len(emb_right) if isinstance(emb_right, (list, tuple)) else 1))
        D = sum(h.out_dim * h.h2 for h in hs)
        if D > _badge.MAX_D:
            raise ValueError("the committee's gradient embedding has D = %d columns (%d members), beyond the %d a picked row may have" % (D, len(hs), _badge.MAX_D))
        torch = hs[0].torch
        embs = []
        for m, h in enumerate(hs):
            L, R = (emb_left[m], emb_right[m]) if per_member else (emb_left, emb_right)
            embs.append(_egl.expected_gradient_length_device(h, L, R, li, ri, want=("emb",))["emb"])
        return _badge.kmeans_pp_device(torch.cat(embs, dim=1), n_instances, uniforms=uniforms, seed=seed)

    def bait_indexed(self, emb_left, emb_right, li, ri, labelled, n_instances, lam=1.0, over=2):
        """Extension: a BAIT batch (bait.py; Ash et al. 2021) of the pairs (li[p], ri[p]) gathered from embedding matrices on device.
        Independent members give a block-diagonal Fisher: a pair's row is the members' Fisher factors side by side (blocks =
        members, at most 512 columns and 8 members) and its score the sum of the members' scores, each against its own A, B.
        `labelled` names the pairs (indices into li / ri, or None) that are labelled already: they enter M0 and are never picked.
        emb_left / emb_right may be lists with one matrix per member, as in egl_indexed.
        -> (idx int32 (k,), score float32 (k,)) on the device, bait.bait_select_device's."""
        from . import bait as _bait, egl as _egl
        hs = self._device_heads()
        if hs is None:
            raise TypeError("bait_indexed needs DenseHead members")
        per_member = isinstance(emb_left, (list, tuple))
        if per_member and (len(emb_left) != len(hs) or not isinstance(emb_right, (list, tuple)) or len(emb_right) != len(hs)):
            raise ValueError("%d members but %d / %d feature matrices" % (len(hs), len(emb_left), len(emb_right) if isinstance(emb_right, (list, tuple)) else 1))
        if len(set(h.h2 for h in hs)) != 1:
            raise ValueError("bait_indexed needs members of one h2: the blocks of a row have one width")
        if len(hs) * hs[0].h2 > _bait.MAX_WIDTH:
            raise ValueError("the committee's Fisher factors have %d columns (%d members x %d), beyond the %d a row may have"
                             % (len(hs) * hs[0].h2, len(hs), hs[0].h2, _bait.MAX_WIDTH))
        _bait._check_shape(hs[0].h2, len(hs))
        torch = hs[0].torch
        fs = []
        for m, h in enumerate(hs):
            L, R = (emb_left[m], emb_right[m]) if per_member else (emb_left, emb_right)
            out = _egl.expected_gradient_length_device(h, L, R, li, ri, want=("probs", "emb"))
            fs.append(_bait.fisher_factor_device(out["probs"], out["emb"]))
        return _bait.bait_factors_device(torch.cat(fs, dim=1), labelled, n_instances, lam=lam, over=over, blocks=len(hs))

    def ranked_batch_indexed(self, emb_left, emb_right, li, ri, labeled, n_instances, kind="entropy", alpha=None):
        """Extension: a ranked batch (batch.py; modAL.batch) of n_instances among the pairs (li[p], ri[p]) gathered from ONE
        left and ONE right embedding matrix on device — the utility weighed against each pair's distance, as the row
        |left - right|, to the labelled rows `labeled` (M, D) and to the picks so far, so near-duplicate pairs do not fill
        the batch.  `kind`: "uncertainty" / "entropy" of predict_indexed's mean (uncertainty.score_device), a kind of
        disagreement_indexed, or "egl" (egl_indexed); "margin" is refused (a SMALLER margin is the more uncertain).  -> (idx int32 (k,), scores (k,))
        on the device, batch.ranked_batch_device's.  Members behind their own feature extractors (lists of matrices) have no
        single row space: score them with disagreement_indexed and call batch.ranked_batch_device on the rows of choice."""
        from . import batch as _batch
        self._one_feature_space(emb_left, emb_right)
        utility = self._indexed_utility(emb_left, emb_right, li, ri, kind)
        return _batch.ranked_batch_device((emb_left, emb_right, li, ri), utility, labeled, n_instances, alpha=alpha)

    @staticmethod
    def _one_feature_space(emb_left, emb_right):
        if isinstance(emb_left, (list, tuple)) or isinstance(emb_right, (list, tuple)):
            raise ValueError("ranked_batch_indexed measures distances in one feature space: one left and one right matrix, not one per member")

    def _indexed_utility(self, emb_left, emb_right, li, ri, kind):
        from . import disagreement as _dis, uncertainty as _unc
        if kind in ("uncertainty", "entropy"):
            return _unc.score_device(self.predict_indexed(emb_left, emb_right, li, ri), kind)
        if kind in _dis.KINDS:
            return self.disagreement_indexed(emb_left, emb_right, li, ri, kind=kind)
        if kind == "egl":
            return self.egl_indexed(emb_left, emb_right, li, ri)
        raise ValueError("unknown utility kind %r: choose among %s (margin: smaller is more uncertain, so it cannot weigh "
                         "against a distance)" % (kind, ["uncertainty", "entropy"] + list(_dis.KINDS) + ["egl"]))

    def density_indexed(self, emb_left, emb_right, li, ri, reference=None):
        """Extension: the information density (density.py; modAL.density) of the pairs (li[p], ri[p]) gathered from ONE left
        and ONE right embedding matrix on device, each pair as the row |left - right| — its mean similarity 1 / (1 + distance)
        to the rows `reference` (R, D), or to all the pairs when reference is None.  -> (N,) float32 on the device,
        density.information_density_device's; weigh a utility with it through density.density_weighted."""
        from . import density as _density
        self._one_feature_space(emb_left, emb_right)
        return _density.information_density_device((emb_left, emb_right, li, ri), reference=reference)["density"]

    def ranked_batch_cold_indexed(self, emb_left, emb_right, li, ri, n_instances, kind="entropy", alpha=None):
        """Extension: ranked_batch_indexed before anything is labelled — the first pick is the pair nearest to all others
        (modAL's cold start), the rest weigh the utility against the distance to it and to the picks so far.  `kind` as in
        ranked_batch_indexed.  -> (idx int32 (k,), scores (k,)) on the device, batch.ranked_batch_cold_device's (scores[0] is NaN)."""
        from . import batch as _batch
        self._one_feature_space(emb_left, emb_right)
        utility = self._indexed_utility(emb_left, emb_right, li, ri, kind)
        return _batch.ranked_batch_cold_device((emb_left, emb_right, li, ri), utility, n_instances, alpha=alpha)

    def kmeans_sampling_indexed(self, emb_left, emb_right, li, ri, n_instances, iters=10, uniforms=None, seed=None):
        """Extension: k-means sampling (cluster.py) of n_instances among the pairs (li[p], ri[p]) gathered from ONE left and ONE
        right embedding matrix on device, each pair as the row |left - right|: the pairs are clustered from k-means++ seeds and
        the pair nearest to each centre is queried.  -> (idx int32 (k,), info) on the device, cluster.kmeans_sampling_device's."""
        from . import cluster as _cluster
        self._one_feature_space(emb_left, emb_right)
        return _cluster.kmeans_sampling_device((emb_left, emb_right, li, ri), n_instances, iters=iters, uniforms=uniforms, seed=seed)

    def diverse_minibatch_indexed(self, emb_left, emb_right, li, ri, n_instances, kind="entropy", beta=10, iters=10, uniforms=None,
                                  seed=None):
        """Extension: a diverse mini-batch (cluster.py; Zhdanov 2019) of n_instances among the pairs (li[p], ri[p]) gathered from
        ONE left and ONE right embedding matrix on device: the beta * k pairs of largest utility, clustered as rows |left - right|
        with the utility as weight, the pair nearest to each centre queried.  `kind` as in ranked_batch_indexed.
        -> (idx int32 (k,), info) on the device, cluster.diverse_minibatch_device's."""
        from . import cluster as _cluster
        self._one_feature_space(emb_left, emb_right)
        utility = self._indexed_utility(emb_left, emb_right, li, ri, kind)
        return _cluster.diverse_minibatch_device((emb_left, emb_right, li, ri), utility, n_instances, beta=beta, iters=iters,
                                                 uniforms=uniforms, seed=seed)

    def typiclust_indexed(self, emb_left, emb_right, li, ri, labelled, n_instances, k_nn=20, min_cluster_size=5, max_clusters=500,
                          iters=10, uniforms=None, seed=None):
        """Extension: TypiClust queries (typiclust.py; Hacohen et al. 2022) among the pairs (li[p], ri[p]) gathered from ONE left
        and ONE right embedding matrix on device, each pair as the row |left - right|; `labelled` names the pairs (indices into
        li / ri) that are labelled already.  The members are not consulted: the strategy needs no scorer.
        -> (picks int64 NumPy array, info), typiclust.typiclust_device's."""
        from . import typiclust as _typiclust
        self._one_feature_space(emb_left, emb_right)
        return _typiclust.typiclust_device((emb_left, emb_right, li, ri), labelled, n_instances, k_nn=k_nn,
                                           min_cluster_size=min_cluster_size, max_clusters=max_clusters, iters=iters, uniforms=uniforms,
                                           seed=seed)

    def probcover_indexed(self, emb_left, emb_right, li, ri, labelled, n_instances, delta=None, groups=None, alpha=0.95, fill=None,
                          random_state=None):
        """Extension: ProbCover queries (probcover.py; Yehuda et al. 2022) among the pairs (li[p], ri[p]) gathered from ONE left
        and ONE right embedding matrix on device, each pair as the row |left - right|; `labelled` names the pairs (indices into
        li / ri) that are labelled already: their balls are covered before the first pick.  delta=None takes the purity radius of
        `groups` (cluster.kmeans_device's "assign" over the same pairs).  The members are not consulted: the strategy needs no
        scorer.  -> (picks int64 NumPy array, info), probcover.probcover_device's."""
        from . import probcover as _probcover
        self._one_feature_space(emb_left, emb_right)
        return _probcover.probcover_device((emb_left, emb_right, li, ri), labelled, n_instances, delta=delta, groups=groups, alpha=alpha,
                                           fill=fill, random_state=random_state)

    def facility_indexed(self, emb_left, emb_right, li, ri, labelled, n_instances, kind=None, beta=10, eps=0.01, cap=None, fill=None,
                         random_state=None):
        """Extension: facility-location queries (facility.py; FASS, Wei, Iyer & Bilmes 2015) among the pairs (li[p], ri[p]) gathered
        from ONE left and ONE right embedding matrix on device, each pair as the row |left - right|; `labelled` names the pairs
        (indices into li / ri) that are labelled already: they are covered before the first pick, so never picked.  kind=None:
        facility location over the whole pool, the members not consulted.  `kind` as in ranked_batch_indexed: FASS — only the
        beta * k unlabelled pairs of largest utility (and the labelled pairs, as labelled) take part.  eps: the stochastic greedy's
        (None: the plain greedy, every pair a candidate at every step).  -> (picks int64 NumPy array, info),
        facility.facility_device's; the picks index li / ri."""
        from . import facility as _facility, uncertainty as _unc
        from .typiclust import _labelled_indices
        self._one_feature_space(emb_left, emb_right)
        pool = (emb_left, emb_right, li, ri)
        if kind is None:
            return _facility.facility_device(pool, labelled, n_instances, cap=cap, eps=eps, fill=fill, random_state=random_state)
        _facility._check_beta(beta)
        torch = self._device_heads()[0].torch
        N = int(li.numel())
        lab = _labelled_indices(labelled, N)
        k = _facility._cluster._check_instances(n_instances)
        utility = self._indexed_utility(emb_left, emb_right, li, ri, kind)
        free = torch.ones(N, dtype=torch.bool, device=li.device)
        lab_t = torch.from_numpy(lab).to(li.device)
        free[lab_t] = False
        unl = torch.nonzero(free).reshape(-1)
        m = int(unl.numel()) if beta is None else min(int(unl.numel()), int(beta) * k)
        if m < 1:
            raise ValueError("facility_indexed: every pair is labelled")
        top = unl.index_select(0, _unc.topk_device(utility.index_select(0, unl), m)[0].long())
        keep = torch.cat([top, lab_t])
        sub = (emb_left, emb_right, li.index_select(0, keep), ri.index_select(0, keep))
        picks, info = _facility.facility_device(sub, np.arange(m, m + len(lab)), n_instances, cap=cap, eps=eps, fill=fill,
                                                random_state=random_state)
        info["kept"] = keep
        return keep.cpu().numpy()[picks].astype(np.int64), info

    def cal_indexed(self, emb_left, emb_right, li, ri, labelled, n_instances, k_nn=10):
        """Extension: Contrastive Active Learning queries (cal.py; Margatina et al. 2021) among the pairs (li[p], ri[p]) gathered
        from ONE left and ONE right embedding matrix on device, each pair as the row |left - right|; `labelled` names the pairs
        (indices into li / ri, at least one) that are labelled already.  A pair's score is the mean KL divergence between the
        committee's mean probabilities (predict_indexed) for its k_nn nearest labelled pairs and for itself; labelled pairs
        are never picked (their scores count as -inf in the top-k).  -> (picks int32 (n,) on the device, info), cal.cal_device's."""
        from . import cal as _cal
        from .typiclust import _labelled_indices
        self._one_feature_space(emb_left, emb_right)
        probs = self.predict_indexed(emb_left, emb_right, li, ri)
        lab = _labelled_indices(labelled, int(li.numel()))
        if len(lab) == 0:
            raise ValueError("cal_indexed needs at least one labelled pair: the score contrasts a pair with its labelled neighbours")
        take = self._device_heads()[0].torch.from_numpy(lab).to(li.device)
        references = (emb_left, emb_right, li.index_select(0, take), ri.index_select(0, take))
        return _cal.cal_device((emb_left, emb_right, li, ri), references, probs, probs.index_select(0, take), n_instances, k_nn=k_nn,
                               exclude=lab)

    def alfamix_indexed(self, emb_left, emb_right, li, ri, labelled, y_labelled, n_instances, eps=0.2, iters=10, seed=None):
        """Extension: ALFA-Mix queries (alfamix.py; Parvaneh et al. 2022) among the pairs (li[p], ri[p]) gathered from ONE left
        and ONE right embedding matrix on device, each pair as the row |left - right|; `labelled` names the pairs (indices into
        li / ri, at least one) that are labelled already and `y_labelled` their classes: the anchors are alfamix.class_anchors
        of those rows (the labelled rows are copied to the host for it).  A candidate is a pair whose decision ANY member flips
        under some anchor — the members' flip masks OR-ed; the fill uses the committee's mean probabilities (predict_indexed);
        labelled pairs are never picked.  -> (picks int32 (n,) on the device, info): alfamix.select_device's picks; info holds
        "flip", "probs" (device) and "anchors" (float32 array)."""
        from . import alfamix as _alfamix
        from .typiclust import _labelled_indices
        self._one_feature_space(emb_left, emb_right)
        hs = self._device_heads()
        if hs is None:
            raise TypeError("alfamix_indexed needs DenseHead members")
        lab = _labelled_indices(labelled, int(li.numel()))
        if len(lab) == 0:
            raise ValueError("alfamix_indexed needs at least one labelled pair: the anchors are the labelled classes' mean rows")
        take = hs[0].torch.from_numpy(lab).to(li.device)
        rows = (emb_left.index_select(0, li.index_select(0, take).long()) - emb_right.index_select(0, ri.index_select(0, take).long())).abs()
        anchors = _alfamix.class_anchors(rows.cpu().numpy(), y_labelled)
        flip = None
        for h in hs:
            f = _alfamix.feature_mix_device(h, emb_left, emb_right, anchors, li, ri, eps=eps, want=("flip",))["flip"]
            flip = f if flip is None else flip | f
        probs = self.predict_indexed(emb_left, emb_right, li, ri)
        picks = _alfamix.select_device((emb_left, emb_right, li, ri), flip, probs, n_instances, iters=iters, seed=seed, exclude=lab)
        return picks, {"flip": flip, "probs": probs, "anchors": anchors}

    def resize(self, images, new_size):
        """cv2.resize(image, new_size) per image (code/committee.py:22-26); new_size = (width, height)."""
        from . import noise as _noise
        out = _noise.resize_images(images, new_size)
        return out if hasattr(out, "detach") else np.array(out)      # CUDA tensors stay on the device

    def attackModel(self, image_pairs, target_size, target_labels=None, rows=None):
        """code/committee.py:28-37: every noise perturbs the pair batch, both sides are resized to
        target_size; returns [[left per noise], [right per noise]].
        rows=(lo, total) (not in the reference): image_pairs / target_labels hold rows lo : lo + len of a batch of
        `total` pairs — one rank's shard; noise objects that take row ranges (noise.py: every one of this package)
        then draw for those rows what the whole-batch call would have drawn, any other duck-typed noise is called the
        reference's way on the rows it is given."""
        sides = ([], [])
        for attack in self.attacks:
            if rows is not None and getattr(attack, "supports_rows", False):
                noisy = attack.addPairNoise(image_pairs, target_labels, rows=rows)
            else:
                noisy = attack.addPairNoise(image_pairs, target_labels)
            for side, images in zip(sides, noisy):
                side.append(self.resize(images, target_size))
        return [sides[0], sides[1]]
