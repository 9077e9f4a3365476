"""The VAEP framework on MI355X (drop-in for ``socceraction.vaep.base``).

``compute_features`` / ``compute_labels`` / ``rate`` keep the reference's per-game
signatures (vaep/base.py:97-137, 296-333) but run as one fused launch each: the game's
actions are flattened once into HBM columns and every known transformer in ``xfns`` is
computed by ``sa_vaep_features`` (windowed game states + left-to-right flip in-kernel).
The ``*_batch`` variants value many games per launch (one segment per game), which is
the throughput path the benchmark measures. ``fit`` / ``score`` delegate to the same
gradient-boosting learners as the reference (host-side, out of the kernel path);
``fit(..., learner='device')`` and ``fit_batch`` train both learners on the device instead
(:mod:`socceraction_amd.boost`).
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
from sklearn.exceptions import NotFittedError
from sklearn.metrics import brier_score_loss, roc_auc_score

from .. import catalog, ops
from .. import spadl as spadlcfg
from ..batch import ActionBatch
from . import features as fs
from . import formula as vaep
from . import labels as lab

try:
    import xgboost
except ImportError:
    xgboost = None  # type: ignore
try:
    import catboost
except ImportError:
    catboost = None  # type: ignore
try:
    import lightgbm
except ImportError:
    lightgbm = None  # type: ignore

xfns_default = [
    fs.actiontype_onehot,
    fs.result_onehot,
    fs.actiontype_result_onehot,
    fs.bodypart_onehot,
    fs.time,
    fs.startlocation,
    fs.endlocation,
    fs.startpolar,
    fs.endpolar,
    fs.movement,
    fs.team,
    fs.time_delta,
    fs.space_delta,
    fs.goalscore,
]


class VAEP:
    """Valuing Actions by Estimating Probabilities (reference vaep/base.py:55-366).

    Parameters
    ----------
    xfns : list
        Feature transformers (default :data:`xfns_default`). Known transformers run in
        the fused HIP kernel; any other callable is evaluated on host game states.
    nb_prev_actions : int, default=3
        Number of previous actions in a game state (1..8 on this backend).
    """

    _spadlcfg = spadlcfg
    _fs = fs
    _lab = lab
    _vaep = vaep
    _atomic = False

    def __init__(self, xfns: Optional[List[Any]] = None, nb_prev_actions: int = 3) -> None:
        self.__models: Dict[str, Any] = {}
        self.xfns = xfns_default if xfns is None else xfns
        self.yfns = [self._lab.scores, self._lab.concedes]
        self.nb_prev_actions = nb_prev_actions

    # ---------------------------------------------------------------- features
    def _split_xfns(self) -> Tuple[List[str], List[Tuple[int, Any]]]:
        known, unknown = [], []
        for i, f in enumerate(self.xfns):
            x = self._fs.xfn_name(f, self._atomic)
            if x is None:
                unknown.append((i, f))
            else:
                known.append(x)
        return known, unknown

    def _host_gamestates(self, actions_with_names: pd.DataFrame, home_team_id):
        gs = self._fs.gamestates(actions_with_names.copy(), self.nb_prev_actions)
        return self._fs.play_left_to_right(gs, home_team_id)

    def _features_frame(self, ab: ActionBatch, actions: pd.DataFrame, homes, segments):
        known, unknown = self._split_xfns()
        parts: Dict[int, pd.DataFrame] = {}
        if known:
            fb = ops.features(ab, known, self.nb_prev_actions)
            kdf = fb.to_frame(index=pd.RangeIndex(ab.n))
        if unknown:  # user transformers: reference semantics on host game states
            named = self._spadlcfg.add_names(actions)
            for i, f in unknown:
                outs = []
                for (s, e), home in zip(segments, homes):
                    gs = self._host_gamestates(named.iloc[s:e].reset_index(drop=True), home)
                    outs.append(f(gs))
                parts[i] = pd.concat(outs, ignore_index=True) if outs else pd.DataFrame()
        if not unknown:
            return kdf
        frames, pos = [], 0
        for i, f in enumerate(self.xfns):
            if i in parts:
                frames.append(parts[i])
            else:
                ncols = len(catalog.xfn_columns(self._fs.xfn_name(f, self._atomic),
                                                self.nb_prev_actions, self._atomic))
                frames.append(kdf.iloc[:, pos:pos + ncols])
                pos += ncols
        return pd.concat(frames, axis=1)

    def compute_features(self, game: pd.Series, game_actions: pd.DataFrame) -> pd.DataFrame:
        """Feature representation of every game state of one game (vaep/base.py:97-116)."""
        home = game.home_team_id
        ab = ActionBatch.from_frame(game_actions, atomic=self._atomic, home_team_id=home)
        return self._features_frame(ab, game_actions, [home], [(0, len(game_actions))])

    def compute_features_batch(self, games: pd.DataFrame, actions: pd.DataFrame) -> pd.DataFrame:
        """Features of many games at once.

        ``actions`` holds the games' actions with each game's rows contiguous;
        ``games`` maps ``game_id -> home_team_id``. Equals ``pd.concat`` of the per-game
        :meth:`compute_features` outputs with ``ignore_index=True``.  With built-in
        transformers only, the pipelined path of :meth:`compute_batch` (features only); with a
        user transformer, one launch for the known ones and the host for the rest.
        """
        if len(actions) and not self._split_xfns()[1]:
            # every transformer a known one: the pipelined path (game-aligned chunks, copies out
            # overlapping the next chunk's encode; socceraction_amd.pipeline), the same frame
            from ..pipeline import value_frames
            return value_frames(self, games, actions, labels=False)[0]
        home_of = games.set_index('game_id')['home_team_id']
        ab = ActionBatch.from_frame(actions, atomic=self._atomic, home_team_id=home_of,
                                    segments='game')
        off = ab.cols['seg_off'].cpu().numpy()
        gids = actions['game_id'].to_numpy()[off[:-1]] if len(actions) else []
        homes = list(home_of.loc[gids]) if len(gids) else []  # one vectorised lookup
        return self._features_frame(ab, actions, homes, list(zip(off[:-1], off[1:])))

    # ---------------------------------------------------------------- labels
    def _labels_frame(self, actions: pd.DataFrame, segments: str) -> pd.DataFrame:
        known = {self._lab.scores: 'scores', self._lab.concedes: 'concedes',
                 self._lab.goal_from_shot: 'goal_from_shot'}
        if all(f in known for f in self.yfns):
            n = len(actions)
            out = {}
            if n:
                ab = ActionBatch.from_frame(actions, atomic=self._atomic, segments=segments)
                lb = ops.labels(ab)
                for f in self.yfns:
                    col = 'goal' if (self._atomic and known[f] == 'goal_from_shot') else known[f]
                    out[col] = getattr(lb, known[f])[:n].cpu().numpy().view(bool)
            else:
                out = {known[f]: np.zeros(0, bool) for f in self.yfns}
            return pd.DataFrame(out, index=pd.RangeIndex(n))
        named = self._spadlcfg.add_names(actions)
        if segments == 'single':
            return pd.concat([fn(named) for fn in self.yfns], axis=1)
        outs = []
        for _, g in named.groupby('game_id', sort=False):
            g = g.reset_index(drop=True)
            outs.append(pd.concat([fn(g) for fn in self.yfns], axis=1))
        return pd.concat(outs, ignore_index=True)

    def compute_labels(self, game: pd.Series, game_actions: pd.DataFrame) -> pd.DataFrame:
        """Labels of every game state of one game (vaep/base.py:118-137)."""
        return self._labels_frame(game_actions, 'single')

    def compute_labels_batch(self, games: pd.DataFrame, actions: pd.DataFrame) -> pd.DataFrame:
        """Labels of many games (contiguous per game) in one launch."""
        return self._labels_frame(actions, 'game')

    def compute_batch(self, games: pd.DataFrame, actions: pd.DataFrame,
                      p_scores=None, p_concedes=None, chunk_rows: int = 1 << 18):
        """``(compute_features_batch, compute_labels_batch, formula values)`` of the same
        games from ONE encode of the frame, pipelined over game-aligned chunks so the host
        encodes the next chunk while the DMA engine copies the last one out
        (:mod:`socceraction_amd.pipeline`).  ``p_scores`` / ``p_concedes``: one probability per
        action (e.g. a fitted model's), else the values are None.  Built-in transformers and
        label functions only."""
        from ..pipeline import value_frames
        return value_frames(self, games, actions, p_scores, p_concedes, chunk_rows)

    # ---------------------------------------------------------------- learning (host)
    def fit(self, X: pd.DataFrame, y: pd.DataFrame, learner: str = 'xgboost',
            val_size: float = 0.25, tree_params: Optional[Dict[str, Any]] = None,
            fit_params: Optional[Dict[str, Any]] = None) -> 'VAEP':
        """Fit one classifier per label (reference vaep/base.py:139-213)."""
        nb_states = len(X)
        idx = np.random.permutation(nb_states)
        train_idx = idx[:math.floor(nb_states * (1 - val_size))]
        val_idx = idx[(math.floor(nb_states * (1 - val_size)) + 1):]
        cols = self._fs.feature_column_names(self.xfns, self.nb_prev_actions)
        if not set(cols).issubset(set(X.columns)):
            missing_cols = ' and '.join(set(cols).difference(X.columns))
            raise ValueError(f'{missing_cols} are not available in the features dataframe')
        if learner == 'device':
            return self._fit_device(X[cols], y, train_idx, val_idx, val_size, tree_params, fit_params)
        X_train, y_train = X.iloc[train_idx][cols], y.iloc[train_idx]
        X_val, y_val = X.iloc[val_idx][cols], y.iloc[val_idx]
        for col in list(y.columns):
            eval_set = [(X_val, y_val[col])] if val_size > 0 else None
            if learner == 'xgboost':
                self.__models[col] = self._fit_xgboost(X_train, y_train[col], eval_set,
                                                       tree_params, fit_params)
            elif learner == 'catboost':
                self.__models[col] = self._fit_catboost(X_train, y_train[col], eval_set,
                                                        tree_params, fit_params)
            elif learner == 'lightgbm':
                self.__models[col] = self._fit_lightgbm(X_train, y_train[col], eval_set,
                                                        tree_params, fit_params)
            else:
                raise ValueError(f'A {learner} learner is not supported')
        return self

    # ---------------------------------------------------------------- learning (device)
    @staticmethod
    def _device_stop_params(early_stopping_rounds, eval_metric, has_val: bool) -> Dict[str, Any]:
        """The device learner's early-stopping parameters, validated before any device call."""
        from .. import boost
        esr, metric = boost.check_stop_params(early_stopping_rounds, eval_metric)
        if esr is not None and not has_val:
            raise ValueError('early_stopping_rounds needs held-out rows: val_size must be positive')
        return dict(early_stopping_rounds=esr, eval_metric=metric)

    def _fit_device(self, X, y, train_idx, val_idx, val_size, tree_params, fit_params=None) -> 'VAEP':
        """``fit(..., learner='device')``: one :class:`socceraction_amd.boost.DeviceGBTClassifier`
        per label column on the reference's split of the rows.  The frame is uploaded and binned
        once (cuts from the training rows).  ``tree_params`` takes the learner's parameters,
        ``subsample``, ``colsample_bytree``, ``reg_alpha``, ``scale_pos_weight`` and ``random_state``
        among them.  ``fit_params`` is read for ``sample_weight`` (row-aligned with ``X``; the
        training rows' weights are used), ``row_keys`` (one integer per row of ``X``, naming the
        rows for ``subsample``; default the row index), ``early_stopping_rounds`` and
        ``eval_metric``: with ``early_stopping_rounds`` the held-out rows are the
        evaluation rows of every round and the best round's model is kept (the reference's
        default ``fit``); without, all trees are trained.  Either way the held-out rows are scored
        once with the kept trees (``self.device_eval_[col]``,
        :func:`socceraction_amd.metrics.binary_scores`)."""
        from .. import boost, metrics
        import torch
        params = boost.check_params(dict(tree_params or {}))  # before any device call
        fp = dict(fit_params or {})
        stop = self._device_stop_params(fp.get('early_stopping_rounds'), fp.get('eval_metric', 'auc'),
                                        val_size > 0 and len(val_idx) > 0)
        train_idx = np.sort(np.asarray(train_idx, np.int64))
        weight, keys = fp.get('sample_weight'), fp.get('row_keys')
        if weight is not None:  # every label's effective weights, before any device call
            for col in list(y.columns):
                weight, _ = boost.check_weights(weight, len(X), y[col].to_numpy(), params['scale_pos_weight'],
                                                train_idx)
        if keys is not None:
            keys = boost.check_row_keys(keys, len(X))
        data = boost.bin_host(X, rows=train_idx)
        rows = torch.from_numpy(train_idx).to(data.device)
        if weight is not None:
            weight = boost.weights_to_device(weight, data.device)
        if keys is not None:
            keys = torch.from_numpy(np.ascontiguousarray(keys)).to(data.device)
        eval_rows = None
        if stop['early_stopping_rounds'] is not None:
            eval_rows = torch.from_numpy(np.sort(np.asarray(val_idx, np.int64))).to(data.device)
        labels = {}
        for col in list(y.columns):
            yh = np.zeros(data.ld, np.uint8)
            yh[:data.n] = y[col].to_numpy().astype(bool)
            labels[col] = torch.from_numpy(yh).to(data.device)
        for col, _, clf in self._fit_labels(labels, params, stop, data, rows, eval_rows, weight, keys):
            if val_size > 0 and len(val_idx):
                p = clf.predict_proba(X.iloc[val_idx])[:, 1]
                self.device_eval_[col] = metrics.binary_scores(y[col].to_numpy().astype(bool)[val_idx], p)
        return self

    def _fit_labels(self, labels, params, stop, data, *fit_args):
        """The per-label tail of both device fits: one classifier per ``labels`` column (name -> device
        labels), kept as its model and yielded with both for the caller's held-out scores."""
        from .. import boost
        self.device_eval_: Dict[str, Dict[str, float]] = {}
        for col, ycol in labels.items():
            self.__models[col] = boost.make_classifier(params, **stop).fit_binned(data, ycol, *fit_args)
            yield col, ycol, self.__models[col]

    def fit_batch(self, games: pd.DataFrame, actions: pd.DataFrame, learner: str = 'device',
                  val_size: float = 0.0, nr_actions: int = 10,
                  tree_params: Optional[Dict[str, Any]] = None,
                  early_stopping_rounds: Optional[int] = None, eval_metric: str = 'auc',
                  sample_weight=None, process_group=None) -> 'VAEP':
        """Fit both learners on many games (contiguous per game) without the feature frame: one
        ``ActionBatch``, the features as bitmaps plus numeric blocks and the labels all on the
        device; only the cut sample and the finished trees cross the link.  ``val_size``: the
        share of rows (the reference's random split) held out and scored once after training
        into ``self.device_eval_``.  ``early_stopping_rounds`` (needs ``val_size > 0``): the
        held-out rows are evaluated after every round by ``eval_metric`` ('auc' or 'logloss')
        and the best round's model is kept.  ``sample_weight``: one weight per row of ``actions``
        (every entry finite and not negative).  With ``subsample`` in ``tree_params`` a round's
        row sample is keyed by ``fm(game_id) + action_id``, built on the device, so it belongs to
        the action, not to its position: the model is the same for any game order or batch
        split (as long as the cuts agree).  Built-in transformers only.

        ``process_group`` (a ``torch.distributed`` group, one process per GPU): every rank passes
        its OWN games and their actions -- for example one range of ``shard.partition_games`` --
        builds its features, labels and bins locally, and both learners are fitted through the
        sharded path (``boost.DeviceGBTClassifier.fit_binned(process_group=)``: the cuts from the
        ranks' global sample, one integer all-reduce per tree level).  Every rank ends with the
        same two models, byte for byte those of one GPU fitted on the ranks' actions in rank
        order, and can ``rate`` its own games.  ``val_size`` splits each rank's own rows, and
        ``device_eval_`` then scores the rank's OWN held-out rows with the common model.
        ``early_stopping_rounds`` needs ``eval_metric='logloss'`` there (the exact AUROC is not
        built across ranks).  A ``ValueError`` on one rank -- an empty ``actions`` frame is one --
        is raised on every rank."""
        from .. import boost, metrics
        from ..trees import TreeEnsemble
        import torch
        group = process_group

        def check():
            if learner != 'device':
                raise ValueError(f'A {learner} learner is not supported by fit_batch')
            params = boost.check_params(dict(tree_params or {}))  # before any device call
            stop = self._device_stop_params(early_stopping_rounds, eval_metric, val_size > 0)
            if group is not None and stop['early_stopping_rounds'] is not None and stop['eval_metric'] != 'logloss':
                raise ValueError("early_stopping_rounds with a process group needs eval_metric='logloss': the "
                                 "exact AUROC is not built across ranks")
            if group is not None and len(actions) == 0:
                raise ValueError('fit_batch with a process group needs actions on every rank')
            weight = sample_weight
            if weight is not None:
                weight, _ = boost.check_weights(weight, len(actions), None, params['scale_pos_weight'])
            sampled = boost.row_threshold(params['subsample']) != boost.THR_ALL
            if sampled and not {'game_id', 'action_id'} <= set(actions.columns):
                raise ValueError('subsample needs the game_id and action_id columns (they key the row sample)')
            known, unknown = self._split_xfns()
            if unknown:
                raise ValueError('fit_batch needs built-in feature transformers')
            return params, stop, weight, sampled, known

        if group is None:
            params, stop, sample_weight, sampled, known = check()
        else:
            err = out = None
            try:
                out = check()
            except ValueError as e:
                err = e
            boost.agree(group, torch.device('cuda', torch.cuda.current_device()), err, 'fit_batch')
            params, stop, sample_weight, sampled, known = out
        home_of = games.set_index('game_id')['home_team_id']
        ab = ActionBatch.from_frame(actions, atomic=self._atomic, home_team_id=home_of, segments='game')
        fb = ops.features(ab, known, self.nb_prev_actions, bool_bits=True)
        lb = ops.labels(ab, int(nr_actions))
        rows = val_rows = None
        if val_size > 0:
            idx = np.random.permutation(ab.n)
            cut = math.floor(ab.n * (1 - val_size))
            rows = torch.from_numpy(np.sort(idx[:cut])).to(ab.device)
            val_rows = torch.from_numpy(np.sort(idx[cut + 1:])).to(ab.device)
        data = boost.bin_blocks(fb, rows=rows, process_group=group)
        keys = boost.row_keys(actions['game_id'].to_numpy(), actions['action_id'].to_numpy(), ab.device) \
            if sampled else None
        if sample_weight is not None:
            sample_weight = boost.weights_to_device(sample_weight, ab.device)
        labels = {col: getattr(lb, col) for col in ('scores', 'concedes')}
        eval_rows = val_rows if stop['early_stopping_rounds'] is not None else None
        for col, ycol, clf in self._fit_labels(labels, params, stop, data, rows, eval_rows, sample_weight, keys, group):
            if val_rows is not None and val_rows.numel():
                p = TreeEnsemble.from_model(clf).predict_blocks(fb)
                self.device_eval_[col] = metrics.binary_scores(ycol[:ab.n][val_rows].contiguous(),
                                                               p[val_rows].contiguous())
        return self

    def _fit_xgboost(self, X, y, eval_set=None, tree_params=None, fit_params=None):
        if xgboost is None:
            raise ImportError('xgboost is not installed.')
        if tree_params is None:
            tree_params = dict(n_estimators=100, max_depth=3)
        if fit_params is None:
            fit_params = dict(eval_metric='auc', verbose=True)
        if eval_set is not None:
            fit_params = {**fit_params, **dict(early_stopping_rounds=10, eval_set=eval_set)}
        return xgboost.XGBClassifier(**tree_params).fit(X, y, **fit_params)

    def _fit_catboost(self, X, y, eval_set=None, tree_params=None, fit_params=None):
        if catboost is None:
            raise ImportError('catboost is not installed.')
        if tree_params is None:
            tree_params = dict(eval_metric='BrierScore', loss_function='Logloss', iterations=100)
        if fit_params is None:
            is_cat_feature = [c.dtype.name == 'category' for (_, c) in X.items()]
            fit_params = dict(cat_features=np.nonzero(is_cat_feature)[0].tolist(), verbose=True)
        if eval_set is not None:
            fit_params = {**fit_params, **dict(early_stopping_rounds=10, eval_set=eval_set)}
        return catboost.CatBoostClassifier(**tree_params).fit(X, y, **fit_params)

    def _fit_lightgbm(self, X, y, eval_set=None, tree_params=None, fit_params=None):
        if lightgbm is None:
            raise ImportError('lightgbm is not installed.')
        if tree_params is None:
            tree_params = dict(n_estimators=100, max_depth=3)
        if fit_params is None:
            fit_params = dict(eval_metric='auc', verbose=True)
        if eval_set is not None:
            fit_params = {**fit_params, **dict(early_stopping_rounds=10, eval_set=eval_set)}
        return lightgbm.LGBMClassifier(**tree_params).fit(X, y, **fit_params)

    def _estimate_probabilities(self, X: pd.DataFrame) -> pd.DataFrame:
        """predict_proba[:, 1] of each fitted model (reference vaep/base.py:284-294)."""
        cols = self._fs.feature_column_names(self.xfns, self.nb_prev_actions)
        if not set(cols).issubset(set(X.columns)):
            missing_cols = ' and '.join(set(cols).difference(X.columns))
            raise ValueError(f'{missing_cols} are not available in the features dataframe')
        Y_hat = pd.DataFrame()
        for col in self.__models:
            Y_hat[col] = [p[1] for p in self.__models[col].predict_proba(X[cols])]
        return Y_hat

    # ---------------------------------------------------------------- rating
    def _device_models(self):
        """The fitted learners as device tree ensembles (socceraction_amd.trees) when every
        one is a supported binary tree model and every transformer is a known one; else None
        (rate then runs the reference's host predict_proba)."""
        from ..trees import TreeEnsemble
        if not {'scores', 'concedes'} <= set(self.__models) or self._split_xfns()[1]:
            return None
        # the cache holds the model objects themselves (compared by identity), so a replaced
        # model can never be mistaken for the cached one through a reused id()
        key = tuple(self.__models.items())
        cached = getattr(self, '_trees_cache', None)
        if cached is not None and len(cached[0]) == len(key) and all(
                c0 == c1 and m0 is m1 for (c0, m0), (c1, m1) in zip(cached[0], key)):
            return cached[1]
        trees = {c: TreeEnsemble.from_model(m) for c, m in self.__models.items()}
        res = trees if all(t is not None for t in trees.values()) else None
        self._trees_cache = (key, res)
        return res

    def _proba_device(self, ab: ActionBatch, trees):
        """features -> predict_proba without leaving HBM: the device probability columns
        ``(p_scores, p_concedes)`` (at least ``ab.n`` rows each). The dtype is the learner's
        (float32 for xgboost, float64 for scikit-learn), as in the reference's host path."""
        import torch
        known, _ = self._split_xfns()
        # the learners read the bool features as bitmaps (64 instead of 515 B/action written);
        # xgboost learners compare float32 values, so their numeric features are written and
        # staged in float32 (half the bytes, the same probabilities bit for bit); better still,
        # their split conditions are evaluated in the numeric pass and only bitmaps are written
        n32 = self.nb_prev_actions <= 3 and all(t.f32 for t in trees.values())
        ps = pc = None
        if n32 and not any(t.le for t in trees.values()):  # xgboost learners: their split conditions evaluated inside the feature passes
            from ..trees import predict_pair_conditions
            try:
                plan = ops.build_plan(known, self.nb_prev_actions, ab.atomic)
                ps, pc = predict_pair_conditions(ab, plan, [trees['scores'], trees['concedes']])
            except ValueError:
                ps = pc = None
        if ps is None and n32:  # float32 numeric blocks, the staged walk over them
            fb = ops.features(ab, known, self.nb_prev_actions, bool_bits=True, num32=True)
            try:
                ps = trees['scores'].predict_blocks(fb)
                pc = trees['concedes'].predict_blocks(fb)
            except ValueError:
                ps = pc = None
        if ps is None:  # a learner whose staged form does not fit LDS: the gather walk, float64 blocks
            fb = ops.features(ab, known, self.nb_prev_actions, bool_bits=True)
            ps = trees['scores'].predict_blocks(fb)
            pc = trees['concedes'].predict_blocks(fb)
        if ps.dtype != pc.dtype:  # pandas would upcast the mixed pair
            ps, pc = ps.to(torch.float64), pc.to(torch.float64)
        return ps, pc

    def _values_device(self, ab: ActionBatch, trees):
        """:meth:`_proba_device` -> formula: the ``[3, ld]`` device tensor of offensive /
        defensive / vaep values, of the probabilities' dtype."""
        ps, pc = self._proba_device(ab, trees)
        return ops.formula(ab, ps, pc)

    def _rate_device(self, ab: ActionBatch, trees) -> pd.DataFrame:
        """:meth:`_values_device`; only the three value columns are copied back."""
        v = self._values_device(ab, trees).cpu().numpy()[:, :ab.n]
        return pd.DataFrame({'offensive_value': v[0], 'defensive_value': v[1],
                             'vaep_value': v[2]})

    def rate(self, game: pd.Series, game_actions: pd.DataFrame,
             game_states: Optional[pd.DataFrame] = None) -> pd.DataFrame:
        """VAEP values of one game's actions (reference vaep/base.py:296-333). Supported
        tree learners (xgboost JSON-dumpable boosters, scikit-learn HistGradientBoosting)
        are evaluated on the device feature blocks when ``game_states`` is not given."""
        if not self.__models:
            raise NotFittedError()
        actions = self._spadlcfg.add_names(game_actions)
        if game_states is None:
            trees = self._device_models()
            if trees is not None:
                ab = ActionBatch.from_frame(game_actions, atomic=self._atomic,
                                            home_team_id=game.home_team_id)
                return self._rate_device(ab, trees)
            game_states = self.compute_features(game, game_actions)
        y_hat = self._estimate_probabilities(game_states)
        return self._vaep.value(actions, y_hat.scores, y_hat.concedes)

    def _probabilities_batch(self, games: pd.DataFrame, actions: pd.DataFrame,
                             game_states: Optional[pd.DataFrame] = None):
        """``(ActionBatch, {label column: device probability column})`` of many games, as
        :meth:`rate_batch` estimates them: supported tree learners on the device feature blocks
        (nothing leaves HBM), any other learner through the feature frame and the host
        ``predict_proba``, its columns uploaded (float32 when the scores / concedes pair is, else float64)."""
        if not self.__models:
            raise NotFittedError()
        if game_states is None:
            trees = self._device_models()
            if trees is not None:
                home_of = games.set_index('game_id')['home_team_id']
                ab = ActionBatch.from_frame(actions, atomic=self._atomic, home_team_id=home_of,
                                            segments='game')
                ps, pc = self._proba_device(ab, trees)
                return ab, {'scores': ps, 'concedes': pc}
            game_states = self.compute_features_batch(games, actions)
        y_hat = self._estimate_probabilities(game_states)
        cols = {c: np.asarray(y_hat[c].to_numpy()) for c in y_hat.columns}
        pair = [cols[c] for c in ('scores', 'concedes') if c in cols] or list(cols.values())
        dt = np.float32 if all(v.dtype == np.float32 for v in pair) else np.float64
        import torch
        ab = ActionBatch.from_frame(actions, atomic=self._atomic, segments='game')
        return ab, {c: torch.from_numpy(np.ascontiguousarray(v, dt)).to(ab.device)
                    for c, v in cols.items()}

    def _values_batch(self, games: pd.DataFrame, actions: pd.DataFrame,
                      game_states: Optional[pd.DataFrame] = None):
        """The ``[3, ld]`` device tensor of :meth:`rate_batch`'s values (offensive, defensive,
        vaep), before its copy back."""
        ab, proba = self._probabilities_batch(games, actions, game_states)
        return ops.formula(ab, proba['scores'], proba['concedes'])

    def rate_batch(self, games: pd.DataFrame, actions: pd.DataFrame,
                   game_states: Optional[pd.DataFrame] = None) -> pd.DataFrame:
        """VAEP values of many games (contiguous per game): one feature launch, one host
        ``predict_proba`` per model, one formula launch with per-game segments."""
        v = self._values_batch(games, actions, game_states).cpu().numpy()[:, :len(actions)]
        return pd.DataFrame({'offensive_value': v[0], 'defensive_value': v[1], 'vaep_value': v[2]})

    def rate_players(self, games: pd.DataFrame, actions: pd.DataFrame, by='player_id',
                     groups=None) -> pd.DataFrame:
        """The rating table of the reference's notebook 4: the values of :meth:`rate_batch`
        summed per ``by`` (a column or a list of columns of ``actions``) with ``count``, as
        ``ratings.group_sums(actions, self.rate_batch(games, actions), by, scale_exp=(2, 2, 2))``
        but without the copy back of the values: they stay in HBM (device learners) or come
        from the host ``predict_proba`` path, go through the order-independent grouped sums
        (|value| <= 2, so the scale exponent is 2) and only the G-row table leaves the device."""
        from .. import ratings
        if not self.__models:
            raise NotFittedError()
        n = len(actions)
        codes, keys = ratings.factorize(actions, by, groups)
        names = ['offensive_value', 'defensive_value', 'vaep_value']
        if len(keys) == 0 or n == 0:  # nothing to rate: the empty table
            return ratings.group_sums(actions, {c: np.zeros(n) for c in names}, by, groups)
        v = self._values_batch(games, actions)
        acc = ratings.sum_device(codes, [v[i, :n] for i in range(3)], len(keys),
                                 scale_exp=(2, 2, 2), dev=v.device)
        return ratings.table(acc, keys, names)

    def top_actions(self, games: pd.DataFrame, actions: pd.DataFrame, k: int = 10,
                    column: str = 'vaep_value', where=None, largest: bool = True) -> pd.DataFrame:
        """The most valuable actions of a selection, the last cell of the reference's notebook 4:
        ``ratings.top_actions(actions, self.rate_batch(games, actions), k, column, where,
        largest)`` -- the ``k`` rows of ``actions`` with the highest (``largest=False``: lowest)
        ``column`` among those ``where`` (a boolean mask per action; None: all) holds, in rank
        order with ``actions``' index, plus ``offensive_value``, ``defensive_value`` and
        ``vaep_value`` -- but without the copy back of every value: the ``[3, ld]`` tensor of
        :meth:`rate_batch`'s path stays in HBM, ``ops.top_rows`` selects on the chosen row (the
        mask is uploaded at one byte per action), and only the selected rows' three values
        leave the device."""
        from .. import ratings
        if not self.__models:
            raise NotFittedError()
        names = ['offensive_value', 'defensive_value', 'vaep_value']
        if column not in names:
            raise ValueError(f'column must be one of {names}')
        n = len(actions)
        if n == 0:
            return ratings.top_actions(actions, {c: np.zeros(0) for c in names}, k, column, where, largest)
        v = self._values_batch(games, actions)
        keep = ratings.mask_tensor(where, n, v.device, actions.index)
        rows, _ = ops.top_rows(v[names.index(column), :n], k, keep, largest)
        sel = v[:, rows].cpu().numpy()
        out = actions.iloc[rows.cpu().numpy()].copy()
        for i, c in enumerate(names):
            out[c] = sel[i]
        return out

    def score(self, X: pd.DataFrame, y: pd.DataFrame) -> Dict[str, Dict[str, float]]:
        """Brier score and AUROC per label (reference vaep/base.py:335-366)."""
        if not self.__models:
            raise NotFittedError()
        y_hat = self._estimate_probabilities(X)
        scores: Dict[str, Dict[str, float]] = {}
        for col in self.__models:
            scores[col] = {}
            scores[col]['brier'] = brier_score_loss(y[col], y_hat[col])
            scores[col]['auroc'] = roc_auc_score(y[col], y_hat[col])
        return scores

    def score_batch(self, games: pd.DataFrame, actions: pd.DataFrame,
                    nr_actions: Optional[int] = None) -> Dict[str, Dict[str, float]]:
        """Brier score, AUROC and log loss per label of the fitted models on many games
        (contiguous per game), with the Brier score and log loss of the base-rate prediction
        (``*_baseline``; the last cell of the reference's notebook 3), without building the
        feature frame: the probabilities of :meth:`rate_batch`'s path and the labels of the same
        encoded batch stay in HBM and go through the order-independent score kernels
        (:func:`socceraction_amd.metrics.binary_scores`); learners the device does not evaluate
        take the feature frame and the host ``predict_proba``, and their probabilities are
        uploaded to the same kernels.  ``nr_actions``: the labels' look-ahead (default 10)."""
        from .. import metrics
        ab, proba = self._probabilities_batch(games, actions)
        lb = ops.labels(ab, 10 if nr_actions is None else int(nr_actions))
        scores: Dict[str, Dict[str, float]] = {}
        for col, p in proba.items():
            name = 'goal_from_shot' if (self._atomic and col == 'goal') else col
            if name not in ('scores', 'concedes', 'goal_from_shot'):
                raise ValueError(f'score_batch knows the labels scores, concedes and goal_from_shot, not {col!r}')
            res = metrics.binary_scores(getattr(lb, name)[:ab.n], p[:ab.n])
            scores[col] = {k: res[k] for k in ('brier', 'auroc', 'log_loss', 'brier_baseline',
                                               'log_loss_baseline')}
        return scores
