"""Entry points with the reference's call signatures for the stages this engine covers:

    from pose2sim_amd import Pose2Sim
    Pose2Sim.synchronization(config)        # reference: Pose2Sim.py:374-376
    Pose2Sim.personAssociation(config)      # reference: Pose2Sim.py:382-384
    Pose2Sim.triangulation(config)          # reference: Pose2Sim.py:386-388

``config`` is None (current directory), a path to a trial / session directory holding Config.toml
files, or an already-merged config dict (Pose2Sim.py:114-162).  Filtering is provided too (see filtering()).  The
other pipeline stages (calibration, pose estimation, marker augmentation, kinematics) are outside this engine's scope
and are not provided: run them with the reference.
"""
import logging
import logging.handlers
import os
import time
from copy import deepcopy
from datetime import datetime

import tomli

# stage name -> (headline of the log banner, module, function, name used in the "... took" line)
_STAGES = {
    'synchronization': ('Camera synchronization', 'synchronization', 'synchronize_cams_all', 'Synchronization'),
    'personAssociation': ('Associating persons', 'personAssociation', 'associate_all', 'Associating persons'),
    'triangulation': ('Triangulation of 2D points', 'triangulation', 'triangulate_all', 'Triangulation'),
    'filtering': ('Filtering 3D coordinates', 'filtering', 'filter_all', 'Filtering'),
}
_OUT_OF_SCOPE = ('calibration', 'poseEstimation', 'markerAugmentation', 'kinematics', 'runAll')


def _load_toml(path):
    with open(path, 'rb') as fh:
        return tomli.load(fh)


def _merged(base, override):
    """A deep copy of `base` with `override` laid over it: tables merge key by key, anything else is replaced
    (what the reference's recursive_update does to its first argument, Pose2Sim.py:78-97)."""
    out = deepcopy(base)
    stack = [(out, override)]
    while stack:
        dst, src = stack.pop()
        for key, value in src.items():
            if isinstance(value, dict) and isinstance(dst.get(key), dict):
                stack.append((dst[key], value))
            else:
                dst[key] = value
    return out


def _config_dirs(top):
    """Directories at or below `top` that hold a Config.toml, in os.walk order with the sub-directories taken by name
    (the reference takes them as the file system lists them, which differs from one machine to the next: a session's
    trials would run in another order there), each with its first file name (the reference opens `files[0]` of such a
    directory, Pose2Sim.py:153) and its depth in path components."""
    found = []
    for root, dirs, files in os.walk(top):
        dirs.sort()                                               # in place: os.walk descends in this order
        if 'Config.toml' in files:
            found.append((root, files[0], len(root.split(os.sep))))
    return found


def read_config_files(config):
    """Pose2Sim.py:100-162 -> (level, [one merged config dict per trial]).

    A dict is taken as it is (level 2).  A directory (None = '.') is a trial when every Config.toml below it sits at one
    depth (level 1: the parent's Config.toml, if readable, is the session default under the trial's own), else a session
    (level 2: its Config.toml under each sub-directory's, trials named in exclude_from_batch left out)."""
    if isinstance(config, dict):
        if config.get('project').get('project_dir') is None:
            logging.warning('Project directory not specified in config dictionary: using current directory.')
        return 2, [config]
    top = '.' if config is None else config
    dirs = _config_dirs(top)
    if not dirs:
        raise FileNotFoundError('You need a Config.toml file in each trial or root folder.')
    depths = [d for _, _, d in dirs]
    level = max(depths) - min(depths) + 1
    if level == 1:
        own = os.path.join(top, 'Config.toml')
        try:
            cfg = _merged(_load_toml(os.path.join(top, '..', 'Config.toml')), _load_toml(own))
        except Exception:
            cfg = _load_toml(own)
        cfg.get('project').update({'project_dir': top})
        return 1, [cfg]
    session = _load_toml(os.path.join(top, 'Config.toml'))
    trials = []
    for root, first_file, _ in dirs:
        if root == top:
            continue
        cfg = _merged(session, _load_toml(os.path.join(root, first_file)))
        cfg.get('project').update({'project_dir': os.path.join(top, os.path.relpath(root))})
        if os.path.basename(root) not in cfg.get('project').get('exclude_from_batch'):
            trials.append(cfg)
    return level, trials


def _session_dir(level):
    """Pose2Sim.py:166-171: the working directory (session level) or its parent (trial level) when it holds a
    calibration folder, else the working directory."""
    cwd = os.getcwd()
    candidate = os.path.realpath(cwd if level == 2 else os.path.join(cwd, '..'))
    try:
        if any('calib' in c.lower() and not c.lower().endswith('.py') for c in os.listdir(candidate)):
            return candidate
    except OSError:
        pass
    return os.path.realpath(cwd)


def _start_logging(session_dir):
    """Pose2Sim.py:69-75: <session>/logs.txt rotated weekly + the console, message-only lines."""
    to_file = logging.handlers.TimedRotatingFileHandler(os.path.join(session_dir, 'logs.txt'), when='D', interval=7)
    logging.basicConfig(format='%(message)s', level=logging.INFO, handlers=[to_file, logging.StreamHandler()])


def _banner(headline, config_dict):
    project_dir = os.path.realpath(config_dict.get('project').get('project_dir'))
    frame_range = config_dict.get('project').get('frame_range')
    which = 'all frames' if not frame_range or frame_range in ('all', 'auto') else f'frames {frame_range[0]} to {frame_range[1]}'
    rule = '---------------------------------------------------------------------'
    for line in ('\n' + rule, f'{headline} for {os.path.basename(project_dir)}, for {which}.',
                 f"On {datetime.now().strftime('%A %d. %B %Y, %H:%M:%S')}", f'Project directory: {project_dir}', rule + '\n'):
        logging.info(line)


def _run_stage(name, config):
    headline, module, function, done = _STAGES[name]
    level, config_dicts = read_config_files(config)
    if not config_dicts[0].get('logging', {}).get('use_custom_logging', False):
        _start_logging(_session_dir(level))
    run = getattr(__import__(f'{__package__}.{module}', fromlist=[function]), function)
    for config_dict in config_dicts:
        _banner(headline, config_dict)
        start = time.time()
        run(config_dict)
        logging.info(f'\n{done} took {time.strftime("%Hh%Mm%Ss", time.gmtime(time.time() - start))}.\n')


def synchronization(config=None):
    """Synchronization of the cameras' JSON files (synchronization.synchronize_cams_all) into pose-sync/; the interactive
    person picker (synchronization_gui = true) is refused with NotImplementedError."""
    _run_stage('synchronization', config)


def personAssociation(config=None):
    _run_stage('personAssociation', config)


def triangulation(config=None):
    _run_stage('triangulation', config)


def filtering(config=None):
    """Filtering of the .trc files (filtering.filter_all): every filter type of the reference's filter_mapping --
    butterworth, butterworth_on_speed, gaussian, median, one_euro, kalman, gcv_spline and loess (the last
    parity-unpinned against statsmodels, which has never run where this was built: filtering.loess_filter)."""
    _run_stage('filtering', config)


def _out_of_scope(name):
    def stage(config=None):
        raise NotImplementedError(f'Pose2Sim.{name}() is outside the scope of this engine (it covers personAssociation, '
                                  'triangulation and Butterworth filtering); run that stage with the reference.')
    stage.__name__ = name
    return stage


for _name in _OUT_OF_SCOPE:
    globals()[_name] = _out_of_scope(_name)
