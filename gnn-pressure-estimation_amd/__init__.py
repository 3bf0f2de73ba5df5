"""MI355X-native GATRes message-passing engine (drop-in for the GATResMeanConv hot path of
DiTEC-project/gnn-pressure-estimation).  See DESIGN.md / INTEGRATION.md at the repository root."""
from . import _native, dp, epoch_control, estimation, evaluation, hydraulics, wdn_io, wdn_synth
from ._build import build_native
from .config_models import config_gatres_large, config_gatres_small, select_model
from .graph_models import GATConv, GATResMeanConv, GResBlockMeanConv, Linear, SimpleConv
from .fused_adam import FusedAdam
from .graph_plan import GraphPlan, PlanCache
from .snapshot_store import SnapshotStore
from .multi_snapshot_store import MultiSnapshotStore
from .train_step import FitHistory, GATResTrainer, internal_train
from .sensor_layout import sensor_layout_draws, sensor_layout_noise
from .estimation import (ErrorBounds, MonitorBaseline, MonitorResult, PressureEstimator, ScreeningBounds, SensitivityMap, conformal_rank, coverage_from_table, greedy_selection,
                         layout_scores_from_table, node_error_bounds, observed_from_names, reading_noise)
from .screening import fault_draws, loo_layouts, loo_residuals_from_estimates, screen_ref, screen_reject_ref, screening_rates
from .monitoring import (cusum_compose, cusum_fixed, cusum_scan_ref, drift_draws, drift_offsets, monitor_baseline_from_moments,
                         monitor_latch_ref, monitor_ref, monitoring_rates)
from .hydraulics import (HydraulicLinksResult, HydraulicNetwork, HydraulicResult, HydraulicSeriesLinksResult, HydraulicSeriesResult,
                         hydraulic_draws, hydraulic_link_draws, hydraulic_residuals, level_update_ref, link_headloss, link_state_ref, pipe_headloss,
                         pump_curve_from_points, series_report, series_valid_ref, series_volume_balance,
                         simulate_series_ref, solve_ref, tree_solution, HydraulicValvesResult, HydraulicSeriesValvesResult,
                         valve_status_ref, hydraulic_valve_draws, HydraulicEmittersResult, HydraulicSeriesEmittersResult,
                         emitter_headloss, hydraulic_emitter_draws, HydraulicPddResult, HydraulicSeriesPddResult, demand_headloss,
                         pdd_lds_bytes, series_pdd_lds_bytes, ControlTable, control_table, control_state,
                         control_step_ref, series_controls_lds_bytes, HydraulicSeriesControlsResult, HydraulicSensitivityResult,
                         LeakLocalization, sensitivity_ref, leak_scores_ref, localization_report, sensitivity_lds_bytes,
                         sensitivity_chunk)
from .wdn_io import parse_inp_hydraulics
from .sensitivity import (influence_from_table, linear_spread_ref, sensitivity_fold_ref, sensitivity_rows_from_gx,
                          sensitivity_seeds)

__all__ = ["FusedAdam", "GATResMeanConv", "GResBlockMeanConv", "GATConv", "SimpleConv", "Linear", "GraphPlan", "PlanCache",
           "GATResTrainer", "FitHistory", "internal_train", "epoch_control", "select_model", "config_gatres_small", "config_gatres_large", "build_native", "wdn_synth", "dp", "evaluation", "wdn_io", "SnapshotStore",
           "MultiSnapshotStore", "estimation", "PressureEstimator", "observed_from_names", "reading_noise",
           "layout_scores_from_table", "greedy_selection", "sensor_layout_draws", "sensor_layout_noise", "ErrorBounds", "conformal_rank",
           "node_error_bounds", "coverage_from_table", "SensitivityMap", "influence_from_table", "linear_spread_ref",
           "sensitivity_fold_ref", "sensitivity_rows_from_gx", "sensitivity_seeds", "ScreeningBounds", "screening", "loo_layouts",
           "loo_residuals_from_estimates", "screen_reject_ref", "screen_ref", "fault_draws", "screening_rates", "MonitorBaseline", "MonitorResult",
           "monitoring", "cusum_scan_ref", "cusum_fixed", "cusum_compose", "monitor_latch_ref", "monitor_ref",
           "monitor_baseline_from_moments", "drift_draws", "drift_offsets", "monitoring_rates", "hydraulics", "HydraulicNetwork",
           "HydraulicResult", "pipe_headloss", "solve_ref", "hydraulic_residuals", "hydraulic_draws", "tree_solution", "HydraulicSeriesResult",
           "simulate_series_ref", "level_update_ref", "series_valid_ref", "series_report", "series_volume_balance",
           "HydraulicLinksResult", "HydraulicSeriesLinksResult", "link_headloss", "link_state_ref", "pump_curve_from_points",
           "hydraulic_link_draws", "parse_inp_hydraulics", "HydraulicValvesResult", "HydraulicSeriesValvesResult", "valve_status_ref",
           "hydraulic_valve_draws", "HydraulicEmittersResult", "HydraulicSeriesEmittersResult", "emitter_headloss",
           "hydraulic_emitter_draws", "HydraulicPddResult", "HydraulicSeriesPddResult", "demand_headloss", "pdd_lds_bytes",
           "series_pdd_lds_bytes", "ControlTable", "control_table", "control_state", "control_step_ref",
           "series_controls_lds_bytes", "HydraulicSeriesControlsResult",
           "HydraulicSensitivityResult", "LeakLocalization", "sensitivity_ref", "leak_scores_ref", "localization_report", "sensitivity_lds_bytes", "sensitivity_chunk"]
