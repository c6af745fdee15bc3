"""Stage 2 of C2-Matching's correspondence training: ``StudentContrasDistillationModel`` (reference:
mmsr/models/student_contras_distillation_model.py, options/train/stage2_student_contras_network.yml).

The student (``net_student``, a ``ContrasExtractorSep`` on the bicubic-upsampled LR input) learns the contrastive hinge
loss of stage 1 plus ``distill_weight`` x KL(teacher || student) of the row-wise softmaxes of the two correlation
matrices at temperature ``temperature``; the frozen stage-1 teacher (``net_teacher``) sees the HR input.  The whole loss
(both dot-product sweeps, the masked arg-mins, the online softmaxes and the KL) runs on the fused gfx950 kernel
(c2m_amd.ops.contras_loss, csrc/contras_loss.hip) for the whole batch.  Option / ``feed_data`` / ``log_dict`` keys,
the ``loss_function`` return tuple, Adam on ``lr_g``, validation and ``save`` (``net_student``) are the reference's.

Deliberate differences from the reference:
  * the teacher runs under ``torch.no_grad()`` and is never wrapped for data parallelism.  The reference runs it with
    gradients enabled and leaves unused ``.grad`` on the teacher's parameters; the student's gradients are the same.
  * ``dist_validation`` calls ``nondist_validation`` (the reference calls a method that does not exist).
LR schedulers are not provided (as in stage 3).
"""
import copy
import logging
from collections import OrderedDict

import torch

import mmsr.models.networks as networks
from mmsr.models.base_model import BaseModel
from mmsr.models.teacher_contras_model import contras_val_loop

logger = logging.getLogger('base')


class StudentContrasDistillationModel(BaseModel):

    def __init__(self, opt):
        super().__init__(opt)
        opt = copy.deepcopy(opt)  # the factories pop 'type'
        self.net_student = self.model_to_device(networks.define_net_student(opt))
        self.net_teacher = self.model_to_device(networks.define_net_teacher(opt), receives_gradients=False)
        for p in self.net_teacher.parameters():
            p.requires_grad = False
        self.net_teacher.eval()
        path = self.opt.get('path') or {}
        strict = path.get('strict_load', True)
        if path.get('pretrain_model_student') is not None:
            self.load_network(self.net_student, path['pretrain_model_student'], strict)
        if path.get('pretrain_model_teacher') is not None:
            self.load_network(self.net_teacher, path['pretrain_model_teacher'], strict)
        if self.is_train:
            self.init_training_settings()

    def init_training_settings(self):
        self.net_student.train()
        self.setup_optimizers()
        self.log_dict = OrderedDict()

    def setup_optimizers(self):
        train_opt = self.opt['train']
        optim_params = []
        for k, v in self.net_student.named_parameters():
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
        self.distill_weight = train_opt.get('distill_weight', 15)
        self.temperature = train_opt.get('temperature', 0.15)

    def feed_data(self, data):
        self.img_in_lq = data['img_in_up'].to(self.device)
        self.img_in_gt = data['img_in'].to(self.device)
        self.img_ref_gt = data['img_ref'].to(self.device)
        self.transformed_coordinates = data['transformed_coordinate'].to(self.device)

    def _teacher_forward(self):
        with torch.no_grad():
            self.teacher_feat = self.net_teacher(self.img_in_gt, self.img_ref_gt)

    def loss_function(self):
        """-> (loss [1], pos_dist, neg_dist, distill_loss), batch means over the samples with >= 128 valid
        correspondences; raises NotImplementedError if there is none (student_contras_distillation_model.py:129-257)."""
        if not hasattr(self, 'margin'):
            self._loss_settings()
        from c2m_amd import ops
        return ops.contras_loss(self.output['dense_features1'], self.output['dense_features2'],
                                self.transformed_coordinates, self.margin, self.safe_radius, self.scaling_steps,
                                teacher=(self.teacher_feat['dense_features1'], self.teacher_feat['dense_features2']),
                                temperature=self.temperature, distill_weight=self.distill_weight)

    def optimize_parameters(self, step):
        self.optimizer_g.zero_grad()
        self.output = self.net_student(self.img_in_lq, self.img_ref_gt)
        self._teacher_forward()
        loss, pos_dist, neg_dist, distill_loss_all = self.loss_function()
        self.log_dict['loss'] = loss.item()
        self.log_dict['pos_dist'] = pos_dist.item()
        self.log_dict['neg_dist'] = neg_dist.item()
        self.log_dict['distill_loss'] = distill_loss_all.item()
        loss.backward()
        self.optimizer_g.step()

    def test(self):
        self.net_student.eval()
        with torch.no_grad():
            self.output = self.net_student(self.img_in_lq, self.img_ref_gt)
        self._teacher_forward()
        self.net_student.train()

    def dist_validation(self, dataloader, current_iter, tb_logger, save_img):
        logger.info('Only support single GPU validation.')
        return self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        return contras_val_loop(self, dataloader, current_iter, tb_logger,
                                ('img_in_lq', 'img_in_gt', 'img_ref_gt', 'transformed_coordinates'),
                                ('loss_val', 'positive_distance', 'negative_distance', 'distill_loss'))

    def save(self, epoch, current_iter):
        self.save_network(self.net_student, 'net_student', current_iter)
        self.save_training_state(epoch, current_iter)
