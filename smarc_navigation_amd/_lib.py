"""ctypes loader for libmcl_hip.so (the C ABI in include/mcl.h, mcl_dr.h, mcl_map.h, mcl_recovery.h, mcl_modes.h,
mcl_history.h, mcl_acoustic.h, mcl_temper.h, mcl_drift.h, mcl_regularise.h, mcl_quantile.h, mcl_innovation.h,
mcl_information.h, mcl_match.h, mcl_swath.h, mcl_reseed.h and mcl_kld.h).

Fails loudly when the shared library is missing: there is no Python/CPU fallback for the hot
path.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C smarc_navigation_amd/csrc`."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('MCL_LIB', os.path.join(_HERE, 'libmcl_hip.so'))  # MCL_LIB: kernel-variant A/B runs

MCL_K_NAMES = ['predict', 'update_gps', 'update_mbes', 'normalise', 'scan', 'resample', 'mean_cov', 'noise', 'comm',
               'mbes_main', 'comm_records', 'pack', 'comm_p2p', 'comm_moments', 'update_landmarks']


class MclError(RuntimeError):
    def __init__(self, status, msg):
        RuntimeError.__init__(self, 'mcl status %d: %s' % (status, msg))
        self.status = status


class Config(C.Structure):
    _fields_ = [('n_particles', C.c_int64), ('n_global', C.c_int64), ('global_offset', C.c_int64),
                ('device', C.c_int32), ('rank', C.c_int32), ('world', C.c_int32),
                ('resample_scheme', C.c_int32), ('rng_mode', C.c_int32), ('comm_mode', C.c_int32),
                ('seed', C.c_uint64), ('init_cov', C.c_double * 6), ('process_cov', C.c_double * 6),
                ('resample_cov', C.c_double * 6), ('meas_std', C.c_double), ('m2o', C.c_double * 16)]


class Odom(C.Structure):
    _fields_ = [('stamp', C.c_double), ('v', C.c_double * 3), ('w_z', C.c_double), ('q', C.c_double * 4),
                ('z', C.c_double)]


class DrConfig(C.Structure):
    _fields_ = [('dvl_period', C.c_double), ('dr_period', C.c_double)]


class DrOdom(C.Structure):
    _fields_ = [('published', C.c_int32), ('used_dvl', C.c_int32), ('t_now', C.c_double), ('pos', C.c_double * 3),
                ('q', C.c_double * 4), ('rpy', C.c_double * 3), ('lin_vel', C.c_double * 3),
                ('ang_vel', C.c_double * 3)]


class Timing(C.Structure):
    _fields_ = [('ms', C.c_double * len(MCL_K_NAMES)), ('launches', C.c_int64 * len(MCL_K_NAMES))]


class Box(C.Structure):
    """mcl_box (include/mcl_recovery.h); frame: 0 = odom, 1 = map"""
    _fields_ = [('x_min', C.c_double), ('x_max', C.c_double), ('y_min', C.c_double), ('y_max', C.c_double),
                ('yaw_min', C.c_double), ('yaw_max', C.c_double), ('frame', C.c_int32)]


class WStats(C.Structure):
    """mcl_wstats (include/mcl_recovery.h)"""
    _fields_ = [('n', C.c_int64), ('n_live', C.c_int64), ('argmax_gid', C.c_int64), ('max_lw', C.c_double),
                ('sum_w', C.c_double), ('sum_w2', C.c_double), ('n_eff', C.c_double), ('log_mean_lik', C.c_double),
                ('map_pose', C.c_double * 6)]


class ModeGrid(C.Structure):
    """mcl_mode_grid (include/mcl_modes.h): the lattice over (x, y, yaw), odom frame"""
    _fields_ = [('x0', C.c_double), ('y0', C.c_double), ('cell', C.c_double), ('nx', C.c_int32), ('ny', C.c_int32),
                ('n_yaw', C.c_int32), ('reserved', C.c_int32)]


class Mode(C.Structure):
    """mcl_mode (include/mcl_modes.h)"""
    _fields_ = [('count', C.c_int64), ('score', C.c_int64), ('ix', C.c_int32), ('iy', C.c_int32), ('iyaw', C.c_int32),
                ('reserved', C.c_int32), ('mean6', C.c_double * 6), ('cov_xy', C.c_double * 3), ('yaw_R', C.c_double)]


class HistoryEst(C.Structure):
    """mcl_history_est (include/mcl_history.h)"""
    _fields_ = [('stamp', C.c_double), ('n_unique', C.c_int64), ('x', C.c_double), ('y', C.c_double), ('yaw', C.c_double),
                ('yaw_R', C.c_double), ('cov_xy', C.c_double * 3)]


class DriftConfig(C.Structure):
    """mcl_drift_config (include/mcl_drift.h)"""
    _fields_ = [('init_std', C.c_double * 3), ('walk_std', C.c_double * 3)]


class RegulariseConfig(C.Structure):
    """mcl_regularise_config (include/mcl_regularise.h)"""
    _fields_ = [('scale', C.c_double), ('shrink', C.c_int32), ('dims', C.c_int32)]


class RegulariseResult(C.Structure):
    """mcl_regularise_result (include/mcl_regularise.h)"""
    _fields_ = [('n', C.c_int64), ('dims', C.c_int32), ('dead', C.c_int32), ('h', C.c_double), ('a', C.c_double),
                ('shift', C.c_double * 6), ('dmean', C.c_double * 6), ('cov', C.c_double * 21), ('chol', C.c_double * 21)]


class TemperRes(C.Structure):
    """mcl_temper_result (include/mcl_temper.h)"""
    _fields_ = [('j', C.c_int32), ('floor_hit', C.c_int32), ('levels_evaluated', C.c_int32), ('reserved', C.c_int32),
                ('n_target', C.c_int64), ('n_live', C.c_int64), ('beta', C.c_double), ('max_lw', C.c_double)]


class QuantileQuery(C.Structure):
    """mcl_quantile_query (include/mcl_quantile.h)"""
    _fields_ = [('quantity', C.c_int32), ('weighted', C.c_int32), ('centre', C.c_double * 3)]


class QuantileResult(C.Structure):
    """mcl_quantile_result (include/mcl_quantile.h)"""
    _fields_ = [('value', C.c_double), ('key', C.c_uint64), ('mass', C.c_uint64), ('total', C.c_uint64),
                ('n_used', C.c_int64)]


class InnovationGateConfig(C.Structure):
    """mcl_innovation_gate_config (include/mcl_innovation.h)"""
    _fields_ = [('nis_gate', C.c_double), ('min_support', C.c_double), ('max_gated_fraction', C.c_double)]


class InnovationVerdict(C.Structure):
    """mcl_innovation_verdict (include/mcl_innovation.h)"""
    _fields_ = [('n_valid', C.c_int32), ('n_candidates', C.c_int32), ('n_gated', C.c_int32), ('inconsistent', C.c_int32),
                ('nis_sum', C.c_double), ('mean_nu', C.c_double)]


# mcl_innovation_beam and mcl_innovation_derived travel as numpy record arrays (40 bytes each): (name, format) pairs
INNOVATION_BEAM_FIELDS = [('n', '<i8'), ('n_miss', '<i8'), ('n_within', '<i8'), ('s1', '<i8'), ('s2', '<u8')]
INNOVATION_DERIVED_FIELDS = [('nu', '<f8'), ('var', '<f8'), ('nis', '<f8'), ('support', '<f8'), ('valid', '<i4'),
                             ('gated', '<i4')]


class InformationSteps(C.Structure):
    """mcl_information_steps (include/mcl_information.h)"""
    _fields_ = [('delta_xy', C.c_double), ('delta_yaw', C.c_double), ('jump_max', C.c_double)]


class MatchConfig(C.Structure):
    """mcl_match_config (include/mcl_match.h)"""
    _fields_ = [('dims', C.c_int32), ('max_iter', C.c_int32), ('min_beams', C.c_int32), ('grad_floor_q', C.c_int32),
                ('step_max_xy', C.c_double), ('step_max_yaw', C.c_double), ('tol_xy', C.c_double), ('tol_yaw', C.c_double),
                ('steps', InformationSteps)]


# mcl_match_sums (152 bytes), mcl_match_result (360), mcl_match_trace (192) and mcl_match_derived_t (192) travel as numpy
# record arrays
MATCH_SUMS_FIELDS = [('n', '<i8'), ('n_miss', '<i8'), ('n_jump', '<i8'), ('S', '<i8', (10,)), ('C', '<i8', (4,)),
                     ('s_rho', '<i8'), ('s_rho2', '<i8')]
MATCH_RESULT_FIELDS = [('x', '<f8'), ('y', '<f8'), ('yaw', '<f8'), ('z', '<f8'), ('status', '<i4'), ('evaluations', '<i4'),
                       ('accepted', '<i4'), ('j', '<i4'), ('dead', '<i4'), ('reserved', '<i4'),
                       ('start', MATCH_SUMS_FIELDS), ('final', MATCH_SUMS_FIELDS)]
MATCH_TRACE_FIELDS = [('x', '<f8'), ('y', '<f8'), ('yaw', '<f8'), ('z', '<f8'), ('sums', MATCH_SUMS_FIELDS), ('j', '<i4'),
                      ('accepted', '<i4')]
MATCH_DERIVED_FIELDS = [('rms', '<f8'), ('mean', '<f8'), ('chi2', '<f8'), ('J', '<f8', (10,)), ('cov', '<f8', (10,)),
                        ('dead', '<i4'), ('m', '<i4')]

# mcl_swath_offset (include/mcl_swath.h; 48 bytes) travels as a numpy record array (engine.SwathOffset is the dtype)
SWATH_OFFSET_FIELDS = [('dx', '<f8'), ('dy', '<f8'), ('dz', '<f8'), ('roll', '<f8'), ('pitch', '<f8'), ('dyaw', '<f8')]

# mcl_reseed_component (include/mcl_reseed.h; 80 bytes) travels as a numpy record array (engine.ReseedComponent is the dtype)
RESEED_COMPONENT_FIELDS = [('mean', '<f8', (3,)), ('chol', '<f8', (6,)), ('mass', '<u4'), ('reserved', '<u4')]


class ReseedSelectConfig(C.Structure):
    """mcl_reseed_select_config (include/mcl_reseed.h)"""
    _fields_ = [('max_components', C.c_int32), ('min_beams', C.c_int32), ('max_rms', C.c_double), ('sep_xy', C.c_double),
                ('sep_yaw', C.c_double), ('cov_scale', C.c_double), ('add_std_xy', C.c_double), ('add_std_yaw', C.c_double),
                ('dead_std_xy', C.c_double), ('dead_std_yaw', C.c_double)]


# mcl_information_sums (72 bytes) and mcl_information_result (104 bytes) travel as numpy record arrays
INFORMATION_SUMS_FIELDS = [('n', '<i8'), ('n_miss', '<i8'), ('n_jump', '<i8'), ('sxx', '<u8'), ('syy', '<u8'), ('sww', '<u8'),
                           ('sxy', '<i8'), ('sxw', '<i8'), ('syw', '<i8')]
INFORMATION_RESULT_FIELDS = [('J', '<f8', (6,)), ('lambda_max', '<f8'), ('lambda_min', '<f8'), ('weak_axis', '<f8'),
                             ('crlb_strong', '<f8'), ('crlb_weak', '<f8'), ('hit_share', '<f8'), ('rank_pos', '<i4'),
                             ('reserved', '<i4')]


# every symbol include/mcl.h, mcl_dr.h and mcl_map.h declare: name -> (restype, argtypes)
_vp, _i32, _i64, _d = C.c_void_p, C.c_int32, C.c_int64, C.c_double
SYMBOLS = {
    'mcl_abi_version': (C.c_int, []),
    'mcl_status_string': (C.c_char_p, [C.c_int]),
    'mcl_last_error': (C.c_char_p, [_vp]),
    'mcl_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'mcl_matrix_from_tf': (C.c_int, [_vp, _vp, _vp]),
    'mcl_create': (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    'mcl_destroy': (C.c_int, [_vp]),
    'mcl_init_particles': (C.c_int, [_vp, _vp]),
    'mcl_predict': (C.c_int, [_vp, C.POINTER(Odom), _d, _vp]),
    'mcl_update_gps': (C.c_int, [_vp, _d, _d]),
    'mcl_set_map_grid': (C.c_int, [_vp, _vp, _i32, _i32, _d, _d, _d]),
    'mcl_set_map_mesh': (C.c_int, [_vp, _vp, _i64, _vp, _i64]),
    'mcl_set_map_mesh_ex': (C.c_int, [_vp, _vp, _i64, _vp, _i64, C.c_uint32]),
    'mcl_update_mbes': (C.c_int, [_vp, _vp, _vp, _i32, _d, _d, _vp]),
    'mcl_mbes_expected': (C.c_int, [_vp, _i64, _i64, _vp, _i32, _d, _vp, _vp]),
    'mcl_update_ranges': (C.c_int, [_vp, _vp, _vp, _i32, _d, _d, _vp, _i32]),
    'mcl_ranges_expected': (C.c_int, [_vp, _i64, _i64, _vp, _i32, _d, _vp, _vp]),
    'mcl_set_landmarks': (C.c_int, [_vp, _vp, _i64]),
    'mcl_set_landmark_noise': (C.c_int, [_vp, _vp, _vp]),
    'mcl_update_landmarks': (C.c_int, [_vp, _vp, _i32, _d, _i32, _d, _vp, _i32]),
    'mcl_update_landmarks_assign': (C.c_int, [_vp, _vp, _i32, _d, _i32, _d, _d, _vp, _i32, _vp, _i64]),
    'mcl_resample': (C.c_int, [_vp, _vp, _i64, _vp]),
    'mcl_resample_prepare': (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    'mcl_mean_cov': (C.c_int, [_vp, _vp, _vp, _vp]),
    'mcl_get_poses': (C.c_int, [_vp, _vp]),
    'mcl_get_particles': (C.c_int, [_vp, _vp, _vp]),
    'mcl_set_particles': (C.c_int, [_vp, _vp]),
    'mcl_get_log_weights': (C.c_int, [_vp, _vp]),
    'mcl_set_log_weights': (C.c_int, [_vp, _vp, _i32]),
    'mcl_get_last_indices': (C.c_int, [_vp, _vp]),
    'mcl_get_last_offspring_cdf': (C.c_int, [_vp, _vp]),
    'mcl_get_fixed_weights': (C.c_int, [_vp, _vp, _vp]),
    'mcl_step_mbes': (C.c_int, [_vp, C.POINTER(Odom), _d, _vp, _vp, _i32, _d, _d, _vp]),
    'mcl_step_mbes_landmarks': (C.c_int, [_vp, C.POINTER(Odom), _d, _vp, _vp, _i32, _d, _d, _vp, _vp, _i32, _d, _i32, _d, _vp]),
    'mcl_sync': (C.c_int, [_vp]),
    'mcl_last_mean_cov': (C.c_int, [_vp, _vp, _vp, _vp]),
    'mcl_mean_history': (C.c_int, [_vp, _i64, _vp]),
    'mcl_resample_indices': (C.c_int, [_i32, _vp, _i64, _vp, _i64, _i32, _vp]),
    'mcl_comm_unique_id': (C.c_int, [C.c_char_p]),
    'mcl_comm_init': (C.c_int, [_vp, C.c_char_p]),
    'mcl_comm_init_ex': (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    'mcl_comm_ranks': (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    'mcl_comm_selftest': (C.c_int, [_vp, _i32]),
    'mcl_comm_shutdown': (C.c_int, [_vp, _i32]),
    'mcl_mean_cov_async': (C.c_int, [_vp]),
    'mcl_group_resample': (C.c_int, [C.POINTER(_vp), _i32, _vp, _i64, C.POINTER(_vp)]),
    'mcl_group_mean_cov': (C.c_int, [C.POINTER(_vp), _i32, _vp, _vp, _vp]),
    'mcl_group_step_mbes': (C.c_int, [C.POINTER(_vp), _i32, C.POINTER(Odom), _d, _vp, _vp, _i32, _d, _d, _vp]),
    'mcl_group_step_mbes_landmarks': (C.c_int, [C.POINTER(_vp), _i32, C.POINTER(Odom), _d, _vp, _vp, _i32, _d, _d, _vp,
                                                _vp, _i32, _d, _i32, _d, _vp]),
    'mcl_exchange_stats': (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32]),
    'mcl_exchange_ops': (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32]),
    'mcl_exchange_plan': (C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    'mcl_timing_enable': (C.c_int, [_vp, _i32]),
    'mcl_timing_get': (C.c_int, [_vp, C.POINTER(Timing)]),
    'mcl_mbes_last_path': (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mcl_mbes_last_handover': (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mcl_mbes_visit_order': (C.c_int, [_vp, _vp, C.POINTER(C.c_int32)]),
    # include/mcl_dr.h: the dead-reckoning integrator (host only)
    'mcl_dr_create': (C.c_int, [C.POINTER(DrConfig), C.POINTER(_vp)]),
    'mcl_dr_destroy': (None, [_vp]),
    'mcl_dr_heading': (C.c_int, [_vp, _vp]),
    'mcl_dr_gps': (C.c_int, [_vp, _d, _d, C.c_int, _vp, C.POINTER(C.c_int), _vp, _vp]),
    'mcl_dr_imu': (C.c_int, [_vp, _d, _vp, _vp]),
    'mcl_dr_dvl': (C.c_int, [_vp, _d, _vp]),
    'mcl_dr_depth': (C.c_int, [_vp, _d]),
    'mcl_dr_thrust_cmd': (C.c_int, [_vp, _d]),
    'mcl_dr_thrust': (C.c_int, [_vp, _d, _d]),
    'mcl_dr_tick': (C.c_int, [_vp, C.POINTER(DrOdom)]),
    'mcl_dr_to_odom': (C.c_int, [C.POINTER(DrOdom), _d, C.POINTER(Odom)]),
    # include/mcl_map.h: the bathymetry map builder
    'mcl_gridmap_create': (C.c_int, [_i32, _i32, _d, _d, _d, _i32, C.POINTER(_vp)]),
    'mcl_gridmap_destroy': (None, [_vp]),
    'mcl_gridmap_last_error': (C.c_char_p, [_vp]),
    'mcl_gridmap_clear': (C.c_int, [_vp]),
    'mcl_gridmap_add_pings': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _d, _vp, _vp, _vp]),
    'mcl_gridmap_finalize': (C.c_int, [_vp, _i32, _vp, C.POINTER(C.c_int64), _vp]),
}

# include/mcl_recovery.h: global localisation and kidnap recovery (a table of its own: SYMBOLS is exactly what the three
# headers above declare)
RECOVERY_SYMBOLS = {
    'mcl_map_bounds': (C.c_int, [_vp, _vp]),
    'mcl_init_particles_uniform': (C.c_int, [_vp, C.POINTER(Box), _vp]),
    'mcl_weight_stats': (C.c_int, [_vp, C.POINTER(WStats)]),
    'mcl_weight_stats_merge': (C.c_int, [C.POINTER(WStats), _i32, C.POINTER(WStats)]),
    'mcl_inject_uniform': (C.c_int, [_vp, _d, C.POINTER(Box), _vp, C.POINTER(C.c_int64)]),
}

# include/mcl_modes.h: the dominant modes of the cloud (a table of its own, like RECOVERY_SYMBOLS)
MODES_SYMBOLS = {
    'mcl_mode_grid_check': (C.c_int, [C.POINTER(ModeGrid), C.POINTER(C.c_int64)]),
    'mcl_pose_modes': (C.c_int, [_vp, C.POINTER(ModeGrid), _i32, C.POINTER(Mode), C.POINTER(_i32), C.POINTER(C.c_int64)]),
}

# include/mcl_history.h: the particle genealogy (a table of its own, like MODES_SYMBOLS)
HISTORY_SYMBOLS = {
    'mcl_history_bytes': (C.c_int, [_i64, _i32, C.POINTER(C.c_int64)]),
    'mcl_history_enable': (C.c_int, [_vp, _i32]),
    'mcl_history_disable': (C.c_int, [_vp]),
    'mcl_history_reset': (C.c_int, [_vp]),
    'mcl_history_record': (C.c_int, [_vp, _d]),
    'mcl_history_frames': (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(C.c_int64), _vp]),
    'mcl_history_ancestors': (C.c_int, [_vp, _i32, _vp]),
    'mcl_history_smooth': (C.c_int, [_vp, _i32, C.POINTER(HistoryEst)]),
    'mcl_history_path': (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
}

# include/mcl_acoustic.h: delayed acoustic position fixes and beacon ranges (a table of its own, like HISTORY_SYMBOLS)
ACOUSTIC_SYMBOLS = {
    'mcl_update_fix': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _d, _i32]),
    'mcl_update_beacon_ranges': (C.c_int, [_vp, _vp, _vp, _i32, _d, _vp, _vp, _i32, _d, _i32]),
    'mcl_history_bracket': (C.c_int, [_vp, _i32, _d, C.POINTER(_i32), C.POINTER(_d), C.POINTER(_i32)]),
}

# include/mcl_temper.h: ESS-targeted likelihood tempering
TEMPER_SYMBOLS = {
    'mcl_temper_beta': (C.c_int, [_i32, C.POINTER(_d)]),
    'mcl_temper_pass': (C.c_int, [C.c_uint64, C.c_uint64, _i64, C.POINTER(_i32)]),
    'mcl_temper_candidates': (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    'mcl_temper': (C.c_int, [_vp, _i64, _i32, C.POINTER(TemperRes)]),
    'mcl_temper_sums': (C.c_int, [_vp, _d, _vp, _i32, _vp, _vp]),
    'mcl_temper_apply': (C.c_int, [_vp, _i32]),
    'mcl_group_temper': (C.c_int, [C.POINTER(_vp), _i32, _i64, _i32, C.POINTER(TemperRes)]),
}

# include/mcl_drift.h: per-particle drift states (water current, yaw-rate bias)
DRIFT_SYMBOLS = {
    'mcl_drift_bytes': (C.c_int, [_i64, C.POINTER(C.c_int64)]),
    'mcl_drift_config_check': (C.c_int, [C.POINTER(DriftConfig), C.POINTER(C.c_char_p)]),
    'mcl_drift_enable': (C.c_int, [_vp, C.POINTER(DriftConfig), _vp]),
    'mcl_drift_reset': (C.c_int, [_vp, _vp]),
    'mcl_drift_disable': (C.c_int, [_vp]),
    'mcl_drift_advance': (C.c_int, [_vp, _d, _vp]),
    'mcl_drift_get': (C.c_int, [_vp, _vp]),
    'mcl_drift_set': (C.c_int, [_vp, _vp]),
    'mcl_drift_mean_cov': (C.c_int, [_vp, _vp, _vp]),
}

# include/mcl_regularise.h: regularised resampling (jitter from the cloud's own covariance)
REGULARISE_SYMBOLS = {
    'mcl_regularise_config_check': (C.c_int, [C.POINTER(RegulariseConfig), C.POINTER(C.c_char_p)]),
    'mcl_regularise_bandwidth': (C.c_int, [_i64, _i32, _d, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'mcl_regularise_factor': (C.c_int, [_vp, _i32, _vp, C.POINTER(C.c_int32)]),
    'mcl_regularise': (C.c_int, [_vp, C.POINTER(RegulariseConfig), _vp]),
    'mcl_regularise_last': (C.c_int, [_vp, C.POINTER(RegulariseResult)]),
}

# include/mcl_quantile.h: exact order statistics of the cloud (median pose, credible radii)
QUANTILE_SYMBOLS = {
    'mcl_quantile_key': (C.c_int, [_d, C.POINTER(C.c_uint64)]),
    'mcl_quantile_value': (C.c_int, [C.c_uint64, C.POINTER(_d)]),
    'mcl_quantile_threshold': (C.c_int, [_d, C.POINTER(C.c_uint64)]),
    'mcl_quantile_reached': (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_i32)]),
    'mcl_cloud_quantiles': (C.c_int, [_vp, C.POINTER(QuantileQuery), _vp, _i32, C.POINTER(QuantileResult)]),
    'mcl_cloud_mass': (C.c_int, [_vp, C.POINTER(QuantileQuery), _d, _vp, _i32, _vp, C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_int64)]),
    'mcl_cloud_key_hist': (C.c_int, [_vp, C.POINTER(QuantileQuery), _d, C.c_uint64, _i32, _vp]),
    'mcl_group_cloud_quantiles': (C.c_int, [C.POINTER(_vp), _i32, C.POINTER(QuantileQuery), _vp, _i32,
                                            C.POINTER(QuantileResult)]),
}

# include/mcl_innovation.h: ping innovation statistics and the per-beam outlier gate
INNOVATION_SYMBOLS = {
    'mcl_innovation_dirs': (C.c_int, [_vp, _i32, _vp]),
    'mcl_innovation_sample': (C.c_int, [_i64, _i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mcl_innovation_merge': (C.c_int, [_vp, _i32, _i32, _vp]),
    'mcl_innovation_gate': (C.c_int, [_vp, _i32, _d, C.POINTER(InnovationGateConfig), _vp, C.POINTER(InnovationVerdict)]),
    'mcl_ping_innovation': (C.c_int, [_vp, _vp, _vp, _i32, _d, _d, _d, _vp, _i32, _vp, _vp, C.POINTER(C.c_int64)]),
    'mcl_group_ping_innovation': (C.c_int, [C.POINTER(_vp), _i32, _vp, _vp, _i32, _d, _d, _d, _vp, _i32, _vp,
                                            C.POINTER(C.c_int64)]),
}

# include/mcl_information.h: ping information, per cloud and per pose
INFORMATION_SYMBOLS = {
    'mcl_information_merge': (C.c_int, [_vp, _i32, _i32, _vp]),
    'mcl_information_matrix': (C.c_int, [_vp, _i32, _i32, _d, _d, _d, _vp]),
    'mcl_ping_information': (C.c_int, [_vp, _vp, _i32, _d, _vp, _i32, C.POINTER(InformationSteps), _vp, _vp,
                                       C.POINTER(C.c_int64)]),
    'mcl_group_ping_information': (C.c_int, [C.POINTER(_vp), _i32, _vp, _i32, _d, _vp, _i32, C.POINTER(InformationSteps), _vp,
                                             C.POINTER(C.c_int64)]),
    'mcl_pose_information': (C.c_int, [_vp, _vp, _i64, _vp, _i32, _d, _vp, C.POINTER(InformationSteps), _vp]),
}

# include/mcl_match.h: ping matching, the pose fix of one ping on the map
MATCH_SYMBOLS = {
    'mcl_match_config_check': (C.c_int, [C.POINTER(MatchConfig), _d, C.POINTER(C.c_char_p)]),
    'mcl_match_solve': (C.c_int, [_vp, C.POINTER(MatchConfig), _i32, _vp, C.POINTER(C.c_int32)]),
    'mcl_match_better': (C.c_int, [_vp, _vp, _i32, C.POINTER(C.c_int32)]),
    'mcl_match_derived': (C.c_int, [_vp, C.POINTER(MatchConfig), _d, _vp]),
    'mcl_match_ping': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _d, _d, _vp, C.POINTER(MatchConfig), _vp, _vp, _vp]),
}

# include/mcl_swath.h: swath matching, the pose fix of the last K pings on the map as one rigid set
SWATH_SYMBOLS = {
    'mcl_swath_offsets': (C.c_int, [_vp, _i32, _i32, _vp]),
    'mcl_swath_check': (C.c_int, [_i32, _i32, _vp, C.POINTER(C.c_char_p)]),
    'mcl_swath_solve': (C.c_int, [_vp, C.POINTER(MatchConfig), _i32, _vp, C.POINTER(C.c_int32)]),
    'mcl_swath_better': (C.c_int, [_vp, _vp, _i32, C.POINTER(C.c_int32)]),
    'mcl_swath_derived': (C.c_int, [_vp, C.POINTER(MatchConfig), _d, _vp]),
    'mcl_match_swath': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _d, _d, _vp, C.POINTER(MatchConfig), _vp, _vp, _vp]),
}

# include/mcl_reseed.h: sensor resetting, particles injected from a mixture of Gaussians at the fixes of a match
RESEED_SYMBOLS = {
    'mcl_reseed_select_check': (C.c_int, [C.POINTER(ReseedSelectConfig), C.POINTER(C.c_char_p)]),
    'mcl_reseed_components_check': (C.c_int, [_vp, _i32, C.POINTER(C.c_char_p)]),
    'mcl_reseed_select': (C.c_int, [_vp, _i64, C.POINTER(MatchConfig), _d, C.POINTER(ReseedSelectConfig), _vp, _vp,
                                    C.POINTER(C.c_int32)]),
    'mcl_inject_gaussian': (C.c_int, [_vp, _d, _vp, _i32, _vp, C.POINTER(C.c_int64)]),
}

# include/mcl_kld.h: KLD-sampling across handles (occupied cells, the bound, the resample from one handle into another)
KLD_SYMBOLS = {
    'mcl_kld_grid_check': (C.c_int, [C.POINTER(ModeGrid), C.POINTER(C.c_int64)]),
    'mcl_kld_bins': (C.c_int, [_vp, C.POINTER(ModeGrid), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mcl_kld_bound': (C.c_int, [_i64, _d, _d, _i64, _i64, C.POINTER(C.c_int64)]),
    'mcl_resample_into': (C.c_int, [_vp, _vp, _vp]),
    'mcl_transfer_last_indices': (C.c_int, [_vp, _vp]),
}

_lib = None


def load():
    """Load libmcl_hip.so and bind every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError('libmcl_hip.so not built (%s): the MCL hot path has no fallback; run '
                          '__graft_entry__.build()' % SO_PATH)
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in (list(SYMBOLS.items()) + list(RECOVERY_SYMBOLS.items()) + list(MODES_SYMBOLS.items()) +
                              list(HISTORY_SYMBOLS.items()) + list(ACOUSTIC_SYMBOLS.items()) +
                              list(TEMPER_SYMBOLS.items()) + list(DRIFT_SYMBOLS.items()) +
                              list(REGULARISE_SYMBOLS.items()) + list(QUANTILE_SYMBOLS.items()) +
                              list(INNOVATION_SYMBOLS.items()) + list(INFORMATION_SYMBOLS.items()) +
                              list(MATCH_SYMBOLS.items()) + list(SWATH_SYMBOLS.items()) + list(RESEED_SYMBOLS.items()) +
                              list(KLD_SYMBOLS.items())):
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.mcl_abi_version() != 4:
        raise ImportError('libmcl_hip.so ABI version mismatch')
    _lib = lib
    return lib


def check(status, handle=None):
    if status != 0:
        lib = load()
        msg = lib.mcl_last_error(handle)
        raise MclError(status, (msg or b'').decode() or lib.mcl_status_string(status).decode())
