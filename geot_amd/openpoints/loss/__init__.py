from .build import (Poly1FocalLoss, Poly1FocalLoss_U, Poly1FocalLoss_U_corr, Poly1FocalLoss_U_T, Weight_CELoss,  # noqa: F401
                    Weight_CELoss_U, build_criterion_from_cfg, criterion_class)
