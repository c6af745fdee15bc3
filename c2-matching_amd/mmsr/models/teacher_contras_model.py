"""Stage 1 of C2-Matching's correspondence training: ``TeacherContrasModel`` (reference:
mmsr/models/teacher_contras_model.py, options/train/stage1_teacher_contras_network.yml).

``net_g`` (a ``ContrasExtractorSep``) maps the HR input and the Ref image to dense features; the contrastive hinge loss
on them (``loss_function``) runs on the fused gfx950 kernel (c2m_amd.ops.contras_loss, csrc/contras_loss.hip) for the
whole batch instead of the reference's per-sample loop of small torch ops.  Option keys, ``feed_data`` keys, the
``loss_function`` return tuple, ``log_dict`` keys, the Adam optimiser on ``lr_g``, validation and ``save`` are the
reference's.  LR schedulers are not provided (as in stage 3).

One fix: the reference's ``dist_validation`` calls a method that does not exist (``self.nondist_val``); here it calls
``nondist_validation``.
"""
import copy
import logging
import os.path as osp
from collections import OrderedDict

import torch

import mmsr.models.networks as networks
from mmsr.models.base_model import BaseModel

logger = logging.getLogger('base')


def contras_val_loop(model, dataloader, current_iter, tb_logger, img_keys, stat_names):
    """Mean of every loss_function() output over a validation loader (teacher_contras_model.py:232-268)."""
    sums = [0.] * len(stat_names)
    count = 0
    dataset_name = getattr(getattr(dataloader, 'dataset', None), 'opt', {}).get('name', 'val')
    for val_data in dataloader:
        model.feed_data(val_data)
        model.test()
        vals = model.loss_function()
        for k in img_keys:
            delattr(model, k)
        del model.output
        for k, v in enumerate(vals):
            sums[k] += float(v)
        count += 1
        if 'name' in val_data:
            logger.debug(f'Test {osp.splitext(osp.basename(val_data["name"][0]))[0]}')
    means = [s / max(count, 1) for s in sums]
    logger.info(f'# Validation {dataset_name} # ' + ' '.join(f'# {n}: {v:.4e}' for n, v in zip(stat_names, means)) + '.')
    if tb_logger:
        tb_logger.add_scalar('loss_val', means[0], current_iter)
    return dict(zip(stat_names, means))


class TeacherContrasModel(BaseModel):

    def __init__(self, opt):
        super().__init__(opt)
        opt = copy.deepcopy(opt)  # the factories pop 'type'
        self.net_g = self.model_to_device(networks.define_net_g(opt))
        path = self.opt.get('path') or {}
        if path.get('pretrain_model_g') is not None:
            self.load_network(self.net_g, path['pretrain_model_g'], path.get('strict_load', True))
        if self.is_train:
            self.init_training_settings()

    def init_training_settings(self):
        self.net_g.train()
        self.setup_optimizers()
        self.log_dict = OrderedDict()

    def setup_optimizers(self):
        train_opt = self.opt['train']
        optim_params = []
        for k, v in self.net_g.named_parameters():
            if v.requires_grad:
                optim_params.append(v)
            else:
                logger.warning(f'Params {k} will not be optimized.')
        self.optimizer_g = torch.optim.Adam(optim_params, lr=train_opt['lr_g'])
        self.optimizers.append(self.optimizer_g)
        self._loss_settings()

    def _loss_settings(self):
        train_opt = self.opt.get('train') or {}
        self.margin = train_opt.get('margin', 1.0)
        self.safe_radius = train_opt.get('safe_radius', 4)
        self.scaling_steps = train_opt.get('scaling_steps', 2)

    def feed_data(self, data):
        self.img_in = data['img_in'].to(self.device)
        self.img_ref = data['img_ref'].to(self.device)
        self.transformed_coordinates = data['transformed_coordinate'].to(self.device)

    def loss_function(self):
        """-> (loss [1], pos_dist, neg_dist), batch means over the samples with >= 128 valid correspondences; raises
        NotImplementedError if there is none (teacher_contras_model.py:115-210)."""
        if not hasattr(self, 'margin'):
            self._loss_settings()
        from c2m_amd import ops
        return ops.contras_loss(self.output['dense_features1'], self.output['dense_features2'],
                                self.transformed_coordinates, self.margin, self.safe_radius, self.scaling_steps)

    def optimize_parameters(self, step):
        self.optimizer_g.zero_grad()
        self.output = self.net_g(self.img_in, self.img_ref)
        loss, pos_dist, neg_dist = self.loss_function()
        self.log_dict['loss'] = loss.item()
        self.log_dict['pos_dist'] = pos_dist.item()
        self.log_dict['neg_dist'] = neg_dist.item()
        loss.backward()
        self.optimizer_g.step()

    def test(self):
        self.net_g.eval()
        with torch.no_grad():
            self.output = self.net_g(self.img_in, self.img_ref)
        self.net_g.train()

    def dist_validation(self, dataloader, current_iter, tb_logger, save_img):
        logger.info('Only support single GPU validation.')
        return self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        return contras_val_loop(self, dataloader, current_iter, tb_logger,
                                ('img_in', 'img_ref', 'transformed_coordinates'),
                                ('loss_val', 'positive_distance', 'negative_distance'))

    def save(self, epoch, current_iter):
        self.save_network(self.net_g, 'net_g', current_iter)
        self.save_training_state(epoch, current_iter)
