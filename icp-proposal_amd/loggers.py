"""Accept/reject JSON log of a chain — writer, reader, best sample, sub-sampling.

Mirrors the reference's on-disk format so that its replay tools can consume chains produced here:
  jsonLogFormat(index, name, logvalue{name -> value}, status, rigid[9], coeff[r], datetime)
      api/sampling/loggers/JSONAcceptRejectLogger.scala:35
  accept: rigid = pose parameters (translation(3), rotation(3), centre(3)), coeff = shape coefficients   :93-98
  reject: EMPTY rigid / coeff, logvalue of the CURRENT state                                           :100-106
  getBestFittingParsFromJSON: accepted record with the largest "product" value                         :142-146
  LogHelper.samplesFromLog (apps/util/LogHelper.scala:27-38): every N-th index, stepping back to the last accepted record.

JSONExperimentLogger (api/sampling/loggers/JSONExperimentLogger.scala) writes the experiment summary of the femur study
(apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:43-64): one jsonExperimentFormat record per init, 17 fields (:29-30).

Input here = the fixed-size per-step records of the host harness (host/icp_host.h): [index, status, leaf id, log value,
theta(10 + r)], which is also what the multi-GPU gather ships.  Host I/O only, but for variability_from_logs, which hands the sub-sampled
states of many logs to the device in one call."""
from __future__ import annotations

import datetime as _dt
import json
import os

import numpy as np


class JSONAcceptRejectLogger:
    def __init__(self, file_path=None):
        self.file_path = file_path
        if file_path is not None:
            parent = os.path.dirname(os.path.abspath(file_path))
            if not os.path.isdir(parent):
                raise IOError(f"JSON log path does not exist: {parent}!")   # :52-54
        self.log_status = []

    # ---- filling
    def add_records(self, records: np.ndarray, leaf_names, evaluator_name: str = "product", logvalues=None):
        """Append the records of icp_host_chain_run (one row per MH step).  `logvalues`: what log_values_of_records gives for these
        records — every record's "logvalue" map then holds all the named evaluators, as the reference's logger writes them (:84-106);
        without it the map holds the record's own value under `evaluator_name`."""
        stamp = _dt.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
        records = np.asarray(records, dtype=np.float64)
        if logvalues is not None and any(len(v) != len(records) for v in logvalues.values()):
            raise ValueError("logvalues: one entry per record under every name")
        for k, rec in enumerate(records):
            accepted = bool(rec[1] != 0.0)
            theta = rec[4:]
            self.log_status.append({
                "index": len(self.log_status),                      # totalSamples at the time of logging (:96,104)
                "name": leaf_names[int(rec[2])],
                "logvalue": ({evaluator_name: float(rec[3])} if logvalues is None
                             else {name: float(v[k]) for name, v in logvalues.items()}),
                "status": accepted,
                # theta = [s | t(3) | phi,theta,psi | centre(3) | c(r)]  ->  rigid = t, rotation, centre (:133-140)
                "rigid": [float(v) for v in theta[1:10]] if accepted else [],
                "coeff": [float(v) for v in theta[10:]] if accepted else [],
                "datetime": stamp,
            })
        return self

    # ---- statistics (:108-110, :148-170)
    @property
    def total_samples(self):
        return len(self.log_status)

    @property
    def percent_accepted(self):
        return sum(1 for r in self.log_status if r["status"]) / max(1, len(self.log_status))

    def percent_accepted_of_type(self, name: str):
        sel = [r for r in self.log_status if r["name"] == name]
        return sum(1 for r in sel if r["status"]) / len(sel) if sel else float("nan")

    # ---- I/O (:112-127)
    def write_log(self):
        with open(self.file_path, "w") as f:
            json.dump(self.log_status, f, indent=2)

    def load_log(self):
        with open(self.file_path) as f:
            return json.load(f)

    @staticmethod
    def sample_to_model_parameters(sample, scale: float = 1.0) -> np.ndarray:
        """jsonLogFormat -> allParameters vector (:133-140); the scale parameter is not logged by the reference."""
        rigid = sample["rigid"]
        return np.concatenate([[scale], rigid[0:3], rigid[3:6], rigid[6:9], sample["coeff"]]).astype(np.float64)

    def get_best_fitting_pars_from_json(self, evaluator_name: str = "product") -> np.ndarray:
        accepted = [r for r in self.load_log() if r["status"]]
        best = max(accepted, key=lambda r: r["logvalue"][evaluator_name])
        return self.sample_to_model_parameters(best)


def samples_from_log(log, take_every_n: int = 50, total: int = 100, burn_in: int = 0):
    """LogHelper.samplesFromLog (apps/util/LogHelper.scala:27-38) — including its use of `total` as the upper index bound."""
    def get_log_index(i):
        while not log[i]["status"]:
            i -= 1
            if i < 0:
                raise IndexError("no accepted sample before the requested index")
        return i
    idx = [get_log_index(i) for i in range(burn_in, min(len(log), total), take_every_n)]
    return [(log[i], i) for i in idx][:min(total, len(idx))]


EVALUATOR_NAMES = ("product", "prior", "distance")  # the map of ProductEvaluators.scala:50-54


def log_values_of_records(records, evaluator, theta_init) -> dict:
    """Every named evaluator on every record of a chain (JSONAcceptRejectLogger.scala:84-106 evaluates the whole map of
    ProductEvaluators.scala:50-54 per logged sample; the step records carry the product alone).  An accepted record is scored at its
    sample, a rejected one at the CURRENT state (:100-106): the last accepted record's state, or `theta_init` before the first
    acceptance.  "distance" comes from ONE api.log_values call over the distinct states under `evaluator` (the chain's likelihood, or
    another one: re-scoring a log), "prior" is the closed form of ModelPriorEvaluator (:24-31), "product" = prior + distance as the
    chain forms it.  Returns {"product", "prior", "distance"}: arrays of one entry per record."""
    from . import api as _api
    records = np.asarray(records, dtype=np.float64)
    if records.ndim != 2:
        raise ValueError("records must be [n_steps, 14 + rank]")
    current = np.ascontiguousarray(theta_init, dtype=np.float64).reshape(-1)
    if records.shape[1] != 4 + current.shape[0]:
        raise ValueError("records and theta_init disagree in the rank")
    states, where, slot = [], {}, np.zeros(len(records), dtype=np.int64)
    for k, rec in enumerate(records):
        if rec[1] != 0.0:
            current = rec[4:]
        key = current.tobytes()
        if key not in where:
            where[key] = len(states)
            states.append(current)
        slot[k] = where[key]
    if not states:
        return {name: np.zeros(0) for name in EVALUATOR_NAMES}
    states = np.stack(states)
    rank = states.shape[1] - 10
    distance = _api.log_values(evaluator, states)["value"]
    # MultivariateNormalDistribution(0, I).logpdf(c), the sum in icp_prior_log_value's order
    nn = np.zeros(len(states))
    for j in range(rank):
        nn += states[:, 10 + j] * states[:, 10 + j]
    prior = -0.5 * nn - 0.5 * rank * np.log(2.0 * np.pi)
    return {"product": (prior + distance)[slot], "prior": prior[slot], "distance": distance[slot]}


def variability_from_logs(contexts, logs, take_every_n: int = 50, total: int = 10000, burn_in: int = 200, mode=(2, 0), theta_refs=None,
                          want_mean: bool = False) -> dict:
    """PosteriorVariabilityToMeshColor (apps/femur/ and apps/bfm/) for many chains: samples_from_log of every log (its defaults here
    are the apps': every 50th state behind a burn-in of 200), logSamples2shapes and the variability maps, in ONE batched device call
    (api.posterior_variability_maps).  `contexts`: one context or one per log; `logs`: per chain the list loadLog gives; `mode`: one
    mode or several — the apps show the normal variance (2, sumNormals = true) and the total variance (0); `theta_refs`: per log, the
    state whose normals mode 1 takes (the apps' best fit).  Returns {"maps": {mode: [one [N] map per log]}, "indices": [per log the
    log indices samples_from_log picked]} and, with want_mean, "means": [per log the [N, 3] mean sample mesh]."""
    from . import api as _api
    logs = list(logs)
    modes = [int(m) for m in mode] if isinstance(mode, (list, tuple)) else [int(mode)]
    if not modes:
        raise ValueError("at least one mode")
    ctxs = list(contexts) if isinstance(contexts, (list, tuple)) else [contexts] * len(logs)
    if len(ctxs) != len(logs):
        raise ValueError("one context per log (or one for all)")
    refs = list(theta_refs) if theta_refs is not None else [None] * len(logs)
    if len(refs) != len(logs):
        raise ValueError("one theta_ref per log")
    picked = [samples_from_log(lg, take_every_n=take_every_n, total=total, burn_in=burn_in) for lg in logs]
    sets = []
    for k, sub in enumerate(picked):
        if len(sub) < 2:
            raise ValueError(f"log {k}: fewer than two samples behind the burn-in")
        sets.append(np.stack([JSONAcceptRejectLogger.sample_to_model_parameters(s) for s, _ in sub]))
    n = len(logs)
    got = _api.posterior_variability_maps(ctxs * len(modes), sets * len(modes), [m for m in modes for _ in range(n)], refs * len(modes),
                                          want_mean=want_mean)
    maps, means = got if want_mean else (got, None)
    out = {"maps": {m: maps[j * n:(j + 1) * n] for j, m in enumerate(modes)}, "indices": [[i for _, i in sub] for sub in picked]}
    if want_mean:
        out["means"] = means[:n]
    return out


def experiment_coefficients(contexts, thetas) -> np.ndarray:
    """The study's model.coefficients(best mesh) (apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala:53-55) for a list of chain
    states, in ONE batched device call (api.model_coefficients): row b is the regularised projection (sigma2 = 1e-5) of the mesh of
    thetas[b] with its own pose taken off — what JSONExperimentLogger.append's coeff* fields hold in the reference.  `contexts`:
    one context or one per state (one model); `thetas`: [n, 10 + rank] with scale 1.  Returns [n, rank]."""
    from . import api as _api
    th = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in thetas]
    return _api.model_coefficients(contexts, thetas=th, poses=[t[:10] for t in th])


# jsonExperimentFormat (api/sampling/loggers/JSONExperimentLogger.scala:29-30), in its field order
EXPERIMENT_FIELDS = ("index", "modelPath", "targetPath", "samplingEuclideanLoggerPath", "samplingHausdorffLoggerPath", "coeffInit",
                     "coeffSamplingEuclidean", "coeffSamplingHausdorff", "coeffIcp", "samplingEuclidean", "samplingHausdorff", "icp",
                     "numOfEvaluationPoints", "numOfSamplePoints", "normalNoise", "datetime", "comment")
EXPERIMENT_DATETIME_FORMAT = "%Y-%m-%d %H:%M:%S"  # SimpleDateFormat("yyyy-MM-dd HH:mm:ss") (:37)
METRIC_KEYS = ("avg", "hausdorff", "dice")  # distMeasure of the study (StdIcpVsChainICPrandomInitComparisonAll.scala:43-50)


class JSONExperimentLogger:
    """api/sampling/loggers/JSONExperimentLogger.scala: the experiment summary (experiments.json) of the femur study.
    The coeff* fields take the coefficient vectors they are given.  The reference logs model.coefficients(mesh), the regularised
    projection (sigma2 = 1e-5) of the best meshes: experiment_coefficients gives those vectors for a list of states in one call
    (theta[10:] itself differs from them by up to 5.8e-6 at rank 201).  The metric maps are keyed avg / hausdorff / dice
    (registration_metrics gives all three)."""

    def __init__(self, file_path, model_path: str = ""):
        self.file_path = str(file_path)
        self.model_path = model_path
        parent = os.path.dirname(os.path.abspath(self.file_path))
        if not os.path.isdir(parent):
            raise IOError(f"JSON log path does not exist: {parent}!")  # :41-43
        if os.path.exists(self.file_path) and not os.access(self.file_path, os.W_OK):
            raise IOError(f"JSON file exist and cannot be overwritten: {self.file_path}!")  # :44-46
        self.experiments = []

    @staticmethod
    def _metrics(m) -> dict:
        return {k: float(v) for k, v in dict(m).items()}

    def append(self, index: int, targetPath: str = "", samplingEuclideanLoggerPath: str = "", samplingHausdorffLoggerPath: str = "",
               coeffInit=(), coeffSamplingEuclidean=(), coeffSamplingHausdorff=(), coeffIcp=(), samplingEuclidean=None,
               samplingHausdorff=None, icp=None, numOfEvaluationPoints: int = 0, numOfSamplePoints: int = 0, normalNoise: float = 0.0,
               comment: str = ""):
        """:63-66; datetime = now, as the reference stamps it."""
        rec = dict(zip(EXPERIMENT_FIELDS, (
            int(index), self.model_path, targetPath, samplingEuclideanLoggerPath, samplingHausdorffLoggerPath,
            [float(v) for v in np.asarray(coeffInit, dtype=np.float64).reshape(-1)],
            [float(v) for v in np.asarray(coeffSamplingEuclidean, dtype=np.float64).reshape(-1)],
            [float(v) for v in np.asarray(coeffSamplingHausdorff, dtype=np.float64).reshape(-1)],
            [float(v) for v in np.asarray(coeffIcp, dtype=np.float64).reshape(-1)],
            self._metrics(samplingEuclidean or {}), self._metrics(samplingHausdorff or {}), self._metrics(icp or {}),
            int(numOfEvaluationPoints), int(numOfSamplePoints), float(normalNoise),
            _dt.datetime.now().strftime(EXPERIMENT_DATETIME_FORMAT), comment)))
        self.experiments.append(rec)
        return rec

    def write_log(self):
        """:69-78 (a JSON list of the records, fields in jsonExperimentFormat order)."""
        with open(self.file_path, "w") as f:
            json.dump(self.experiments, f, indent=2)

    def load_log(self):
        """:81-84"""
        with open(self.file_path) as f:
            return json.load(f)


def distance_summaries_from_logs(contexts, logs, take_every_n: int = 50, total: int = 10000, burn_in: int = 200,
                                 want=("m2t_mean", "m2t_max", "t2m_mean", "t2m_max")) -> dict:
    """The distance maps many chains' logs imply: samples_from_log of every log (variability_from_logs' defaults), logSamples2shapes
    and, in ONE batched device call (api.distance_summaries), per vertex the mean and the maximum over the picked states of the
    distance to the target's surface — and of every target vertex's distance to the sample's surface.  `contexts`: one context or one
    per log; `logs`: per chain the list loadLog gives.  Returns {"summaries": [per log api.distance_summaries' dict], "indices": [per
    log the log indices samples_from_log picked]}."""
    from . import api as _api
    logs = list(logs)
    ctxs = list(contexts) if isinstance(contexts, (list, tuple)) else [contexts] * len(logs)
    if len(ctxs) != len(logs):
        raise ValueError("one context per log (or one for all)")
    picked = [samples_from_log(lg, take_every_n=take_every_n, total=total, burn_in=burn_in) for lg in logs]
    sets = []
    for k, sub in enumerate(picked):
        if len(sub) < 1:
            raise ValueError(f"log {k}: no sample behind the burn-in")
        sets.append(np.stack([JSONAcceptRejectLogger.sample_to_model_parameters(s) for s, _ in sub]))
    return {"summaries": _api.distance_summaries(ctxs, sets, want=want), "indices": [[i for _, i in sub] for sub in picked]}
