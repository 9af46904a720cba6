"""Configuration object with the attribute names of the reference's utils/config.py.

The hot-path code reads ``config.<name>`` exactly like the reference's blocks / datasets do
(models/blocks.py:523-544, datasets/common.py:468,501,518), so a reference ``Config`` subclass
(e.g. train_DALES_PseudoLabel.py:44-201) can be passed in unchanged; this class exists so that
the package is usable without the reference tree.  Defaults follow utils/config.py:35-189; the
derived fields follow Config.__init__ (:191-233).  `save()` / `load(path)` write and read the reference's
parameters.txt (:235-445): the same keys, order, sections and number formats, so a file of either side loads in the
other and load followed by save reproduces it.
"""
import os

import numpy as np

# parameters.txt as a table: sections of (attribute, kind, blank lines after).  Kinds: s string, d integer, b boolean
# written 0 / 1, f float with six decimals, f3 with three, bs / fs / ss lists, D integer or None, N integer or list of
# integers (num_classes), L the {epoch: factor} dictionary.  num_layers is derived: written, not read.
_SECTIONS = (
    ('Input parameters', '****************', (
        ('dataset', 's', 0), ('dataset_task', 's', 0), ('num_classes', 'N', 0), ('in_points_dim', 'd', 0),
        ('in_features_dim', 'd', 0), ('in_radius', 'f', 0), ('input_threads', 'd', 1))),
    ('Model parameters', '****************', (
        ('architecture', 'ss', 0), ('equivar_mode', 's', 0), ('invar_mode', 's', 0), ('num_layers', 'd', 0),
        ('first_features_dim', 'd', 0), ('use_batch_norm', 'b', 0), ('batch_norm_momentum', 'f', 1),
        ('segmentation_ratio', 'f', 1))),
    ('KPConv parameters', '*****************', (
        ('first_subsampling_dl', 'f', 0), ('num_kernel_points', 'd', 0), ('conv_radius', 'f', 0), ('deform_radius', 'f', 0),
        ('fixed_kernel_points', 's', 0), ('KP_extent', 'f', 0), ('KP_influence', 's', 0), ('aggregation_mode', 's', 0),
        ('modulated', 'b', 0), ('n_frames', 'd', 0), ('max_in_points', 'd', 1), ('max_val_points', 'd', 1),
        ('val_radius', 'f', 1))),
    ('Training parameters', '*******************', (
        ('learning_rate', 'f', 0), ('momentum', 'f', 0), ('lr_decays', 'L', 0), ('grad_clip_norm', 'f', 1),
        ('augment_symmetries', 'bs', 0), ('augment_rotation', 's', 0), ('augment_noise', 'f', 0),
        ('augment_occlusion', 's', 0), ('augment_occlusion_ratio', 'f', 0), ('augment_occlusion_num', 'd', 0),
        ('augment_scale_anisotropic', 'b', 0), ('augment_scale_min', 'f', 0), ('augment_scale_max', 'f', 0),
        ('augment_color', 'f', 1),
        ('weight_decay', 'f', 0), ('segloss_balance', 's', 0), ('class_w', 'fs', 0), ('deform_fitting_mode', 's', 0),
        ('deform_fitting_power', 'f', 0), ('deform_lr_factor', 'f', 0), ('repulse_extent', 'f', 0), ('batch_num', 'd', 0),
        ('val_batch_num', 'd', 0), ('max_epoch', 'd', 0), ('epoch_steps', 'D', 0), ('validation_size', 'd', 0),
        ('checkpoint_gap', 'd', 1))),
)
# the last section: a line only when the configuration has the attribute (:420-445)
_OTHER = (('sub_radius', 'f'), ('model_name', 's'), ('loss_type', 's'), ('contrast_start', 'f'), ('contrast_thd', 'f'),
          ('anchor_method', 's'), ('active_learning_iterations', 'd'), ('subsample_labels', 'b'),
          ('initial_labels_per_file', 'd'), ('subsample_method', 's'), ('added_labels_per_epoch', 'd'),
          ('weak_label_log', 's'), ('dropout', 'f3'),
          ('batch_norm_mode', 's'),      # 'reference' (the identity of blocks.py:453-463, also when absent) | 'points': no class declares it
          ('batch_norm_sync', 'b'),      # 'points' under data parallelism: batch statistics over all ranks (dp.sync_batch_norm); absent = off: no class declares it
          ('al_min_spacing', 'f'))       # minimum distance between new active-learning labels and to the used ones (active.spaced_top_k); absent or 0 = off: no class declares it
_FILE_KEY = {'lr_decays': 'lr_decay_epochs', 'contrast_thd': 'contrast_thd[%]'}        # attribute -> its key in the file
_DERIVED = ('num_layers',)
_ONE = {'s': '{:s}', 'd': '{:d}', 'f': '{:.6f}', 'f3': '{:.3f}'}


def _write_value(kind, v):
    """the text behind `key =`, leading blank included (a list without members leaves the bare `key =`)"""
    if kind == 'b':
        return ' {:d}'.format(int(v))
    if kind in _ONE:
        return ' ' + _ONE[kind].format(v)
    if kind == 'D':
        return ' None' if v is None else ' {:d}'.format(v)
    if kind == 'N':
        return ''.join(' {:d}'.format(n) for n in v) if type(v) is list else ' {:d}'.format(v)
    if kind == 'L':
        return ''.join(' {:d}:{:f}'.format(e, d) for e, d in v.items())
    if kind == 'bs':
        return ''.join(' {:d}'.format(int(a)) for a in v)
    return ''.join(' ' + _ONE[kind[0]].format(a) for a in v)             # ss, fs


def _read_value(kind, words):
    """words: what follows `key =`, at least one"""
    if kind == 'N':
        return [int(c) for c in words] if len(words) > 1 else int(words[0])
    if kind == 'L':
        return {int(b.split(':')[0]): float(b.split(':')[1]) for b in words}
    if kind == 'bs':
        return [bool(int(b)) for b in words]
    if kind in ('ss', 'fs'):
        return [{'s': str, 'f': float}[kind[0]](w) for w in words]
    w = words[0]
    if kind == 'b':
        return bool(int(w))
    if kind in ('d', 'D'):
        return float(w) if len(w.split('.')) == 2 else int(w)           # (the reference's rule: one dot makes a float)
    return float(w) if kind in ('f', 'f3') else w


class Config:
    # ---- input
    dataset = ''
    dataset_task = ''
    num_classes = 0
    in_points_dim = 3
    in_features_dim = 1
    in_radius = 1.0
    input_threads = 8
    # ---- model
    architecture = []
    equivar_mode = ''
    invar_mode = ''
    first_features_dim = 64
    use_batch_norm = True
    batch_norm_momentum = 0.99
    segmentation_ratio = 1.0
    # ---- KPConv
    num_kernel_points = 15
    first_subsampling_dl = 0.02
    conv_radius = 2.5
    deform_radius = 5.0
    KP_extent = 1.0
    KP_influence = 'linear'
    aggregation_mode = 'sum'
    fixed_kernel_points = 'center'
    modulated = False
    n_frames = 1
    max_in_points = 0
    val_radius = 51.0
    max_val_points = 50000
    # ---- training
    learning_rate = 1e-3
    momentum = 0.9
    lr_decays = {200: 0.2, 300: 0.2}
    grad_clip_norm = 100.0
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [False, False, False]
    augment_rotation = 'vertical'
    augment_noise = 0.005
    augment_color = 0.7
    augment_occlusion = 'none'
    augment_occlusion_ratio = 0.2
    augment_occlusion_num = 1
    weight_decay = 1e-3
    segloss_balance = 'none'
    class_w = []
    deform_fitting_mode = 'point2point'
    deform_fitting_power = 1.0
    deform_lr_factor = 0.1
    repulse_extent = 1.0
    batch_num = 10
    val_batch_num = 10
    max_epoch = 1000
    epoch_steps = 1000
    validation_size = 100
    checkpoint_gap = 50
    dropout = 0
    saving = True
    saving_path = None

    def __init__(self):
        arch = self.architecture
        self.num_layers = len([b for b in arch if 'pool' in b or 'strided' in b]) + 1
        # which layers contain a deformable convolution (utils/config.py:197-233)
        self.deform_layers = []
        layer_blocks = []
        for block in arch:
            if not any(tag in block for tag in ('pool', 'strided', 'global', 'upsample')):
                layer_blocks.append(block)
                continue
            deform = bool(layer_blocks) and bool(np.any(['deformable' in b for b in layer_blocks]))
            if ('pool' in block or 'strided' in block) and 'deformable' in block:
                deform = True
            self.deform_layers.append(deform)
            layer_blocks = []
            if 'global' in block or 'upsample' in block:
                break

    def save(self):
        """write `saving_path`/parameters.txt (utils/config.py:311-445)"""
        out = ['# -----------------------------------#\n', '# Parameters of the training session #\n',
               '# -----------------------------------#\n\n']
        for title, rule, entries in _SECTIONS:
            out.append('# %s\n# %s\n\n' % (title, rule))
            for attr, kind, blanks in entries:
                out.append(_FILE_KEY.get(attr, attr) + ' =' + _write_value(kind, getattr(self, attr)) + '\n' * (1 + blanks))
        out.append('# Other parameters\n# *******************\n\n')
        absent = getattr(self, '_absent_when_loaded', {})
        for attr, kind in _OTHER:
            if hasattr(self, attr) and not (attr in absent and absent[attr] == getattr(self, attr)):
                out.append(_FILE_KEY.get(attr, attr) + ' =' + _write_value(kind, getattr(self, attr)) + '\n')
        with open(os.path.join(self.saving_path, 'parameters.txt'), 'w') as f:
            f.write(''.join(out))

    def load(self, path):
        """read parameters.txt (utils/config.py:235-309).  path: the log directory, or the file itself.  Every key of the
        table is read with its own type, whether or not this object had the attribute (the reference drops the optional
        keys of a class that does not declare them, and `contrast_thd[%]` always); any other key is taken only when the
        attribute exists, with the reference's typing.  `key = None` gives None; a bare `key =` empties a list or the decay dictionary
        (the reference keeps the class default there) and leaves a string alone.
        As there: saving = True, saving_path = the directory, and the derived fields are computed again.  -> self"""
        filename = os.path.join(path, 'parameters.txt') if os.path.isdir(path) else path
        kinds = {_FILE_KEY.get(a, a): (a, k) for _, _, entries in _SECTIONS for a, k, _ in entries}
        kinds.update({_FILE_KEY.get(a, a): (a, k) for a, k in _OTHER})
        with open(filename, 'r') as f:
            lines = f.readlines()
        seen = set()
        for line in lines:
            words = line.split()
            if len(words) < 2 or words[0] == '#' or words[1] != '=':
                continue
            seen.add(words[0])
            if len(words) == 2 and kinds.get(words[0], ('', ''))[1] in ('ss', 'fs', 'bs', 'L'):
                setattr(self, kinds[words[0]][0], {} if kinds[words[0]][1] == 'L' else [])      # a list without members
            if len(words) < 3 or words[0] in _DERIVED:
                continue
            key, values = words[0], words[2:]
            if values[0] == 'None':
                setattr(self, kinds[key][0] if key in kinds else key, None)
            elif key in kinds:
                setattr(self, kinds[key][0], _read_value(kinds[key][1], values))
            elif hasattr(self, key):
                kind = float if len(values[0].split('.')) == 2 else type(getattr(self, key))
                setattr(self, key, bool(int(values[0])) if kind is bool else kind(values[0]))
        # an optional attribute this class declares (`dropout`) but the file does not name: save() leaves its line out for
        # as long as the value stays what it is now, so that load followed by save reproduces the file
        self._absent_when_loaded = {a: getattr(self, a) for a, _ in _OTHER if hasattr(self, a) and _FILE_KEY.get(a, a) not in seen}
        self.saving = True
        self.saving_path = os.path.dirname(os.path.abspath(filename))
        Config.__init__(self)
        return self


_PL_ARCH = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
            'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
            'nearest_upsample', 'unary', 'nearest_upsample', 'unary',
            'nearest_upsample', 'unary', 'nearest_upsample', 'unary']


class DALESPLConfig(Config):
    """values of train_DALES_PseudoLabel.py:44-201 that reach the hot path"""
    dataset = 'DALESPL'
    contrast_start = 0        # train_DALES_PseudoLabel.py:181-182
    contrast_thd = 10
    input_threads = 10
    architecture = list(_PL_ARCH)
    num_kernel_points = 15
    in_radius = 18
    first_subsampling_dl = 0.4
    conv_radius = 2.5
    deform_radius = 5.0
    KP_extent = 1.0
    first_features_dim = 128
    in_features_dim = 3
    modulated = False
    use_batch_norm = True
    batch_norm_momentum = 0.02
    repulse_extent = 1.2
    learning_rate = 0.001
    momentum = 0.98
    grad_clip_norm = 100.0
    batch_num = 4
    dropout = 0.5
    class_w = [1, 1, 1, 1, 1, 1, 1, 1, 1]


class Vaihingen3DPLConfig(Config):
    """values of train_Vaihingen3D_PseudoLabel.py that reach the hot path"""
    dataset = 'Vaihingen3DPL'
    input_threads = 10
    architecture = list(_PL_ARCH)
    num_kernel_points = 15
    in_radius = 24
    first_subsampling_dl = 0.24
    conv_radius = 2.5
    deform_radius = 6.0
    KP_extent = 1.0
    first_features_dim = 64
    in_features_dim = 4
    modulated = False
    use_batch_norm = True
    batch_norm_momentum = 0.02
    repulse_extent = 1.2
    learning_rate = 0.01
    momentum = 0.98
    grad_clip_norm = 100.0
    batch_num = 4
    dropout = 0.5
    class_w = [1, 1, 1, 1, 1, 1, 1, 1, 1]


class DALESDeformConfig(DALESPLConfig):
    """BASELINE config 5 as SURVEY.md section 8d specifies it: the DALES network with every `resnetb` block replaced by
    `resnetb_deformable` (learned offsets, models/blocks.py:244-325) and `modulated = True` (:256,:366-367),
    deform_radius 5.0 -- so every level is searched with the deformable radius r * deform_radius / conv_radius = 2 r
    (datasets/common.py:498-503: about 8 x the neighbours) -- and feature rows / weights bf16 with fp32 accumulate
    (`feature_dtype`; the reference has no reduced-precision path: fp32 masters, bf16 rows in HBM)."""
    dataset = 'DALESDeform'
    architecture = [b.replace('resnetb', 'resnetb_deformable') for b in _PL_ARCH]
    modulated = True
    deform_radius = 5.0
    feature_dtype = 'bf16'


class DALESDeformF32Config(DALESDeformConfig):
    """the same network with f32 rows (A/B of the bf16 path; oracle comparisons at 1e-4)"""
    dataset = 'DALESDeformF32'
    feature_dtype = 'f32'


_WL_ARCH = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
            'nearest_upsample', 'nearest_upsample']


class Vaihingen3DWLConfig(Config):
    """values of train_Vaihingen3D_WeakLabel.py:46-178 that reach the weak-label step (BASELINE config 1): the 3-layer
    multi-path region-mining network KPFCNN_mprm, 64 first features, dl0 0.24, the region loss, gradient-NORM clipping at 1"""
    dataset = 'Vaihingen3DWL'
    input_threads = 10
    architecture = list(_WL_ARCH)
    num_kernel_points = 15
    in_radius = 18
    sub_radius = 5
    first_subsampling_dl = 0.24
    conv_radius = 2.5
    deform_radius = 1.0
    KP_extent = 1.0
    KP_influence = 'linear'
    aggregation_mode = 'sum'
    first_features_dim = 64
    in_features_dim = 4
    modulated = False
    use_batch_norm = True
    batch_norm_momentum = 0.02
    deform_fitting_mode = 'point2point'
    deform_fitting_power = 1.0
    deform_lr_factor = 0.1
    repulse_extent = 1.2
    max_epoch = 80
    learning_rate = 0.01
    momentum = 0.98
    lr_decays = {i: 0.98 for i in range(1, 1000)}
    grad_clip_norm = 1
    batch_num = 3
    class_w = [1, 1, 1, 1, 1, 1, 1, 1, 1]
    num_classes = 9
    model_name = 'KPFCNN_mprm'
    loss_type = 'region_mprm_loss'
    anchor_method = 'reduced'
