// SMP_families_hip.h -- drop-ins for the public training / inference API of the reference's single-handle model classes that came after
// SMP_omega: one thin class per reference class on the skeleton of SMP_handle_hip.h, each with that class's constructor argument list
// (GraphFlow/<class>.h), its optimiser, and its initial weights from rand() after the caller's srand().  The configuration of each
// family is the one graphflow_amd/smp.py's config() methods build (include/gf_hip.h: gf_smp_config).
//
//   first order          SMP_theta (Adam); SMP_1D, SMP_1D_ver2, SMP_1D_ver3, SMP_1D_classification, SMP_1D_ver3_classification
//   steerable 2nd order  SMP_2D, SMP_2D_ver4, SMP_2D_ver5, SMP_2D_classification, SMP_2D_ver4_classification
//   unrestricted         Unrestricted_SMP_1D, Unrestricted_SMP_1D_ver2, Unrestricted_SMP_2D
//   neighbourhood        NeuralFingerprint, GCN_1D, GCN_2D, GCN_3D;  gated: GRU_GCN_1D, GRU_GCN_2D, GRU_GCN_3D
//   distance             GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance          (read molecule->distance)
//   pairs / Gram         GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (two graphs per sample);  GCA_1D (no target)
//   matrix form          LCNN, GCN_MW
//   covariant            CGCN_1D, CGCN_2D
// Every class but SMP_theta trains with Momentum(momentum_param).  Not here, as in the library: SMP_2D_ver2 / ver3 and
// Unrestricted_SMP_2D_ver2 (ill-defined in the reference), and towers or data-parallel steps of these forms.
#ifndef GF_SMP_FAMILIES_HIP_H_INCLUDED
#define GF_SMP_FAMILIES_HIP_H_INCLUDED

#include "SMP_handle_hip.h"

namespace gfhost {

// the field-level families: receptive fields without a cap (max_receptive_field = max_nVertices)
inline gf_smp_config field_config(int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, bool has_WL_ordering) {
    gf_smp_config c = zero_config();
    c.nLevels = nLevels;
    c.nChanels = nChanels;
    c.nFeatures = nFeatures;
    c.nDepth = nDepth;
    c.max_receptive_field = c.max_nVertices = max_nVertices;
    c.has_WL_ordering = has_WL_ordering ? 1 : 0;
    return c;
}
inline gf_smp_config first_order_config(int form, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, bool wl) {
    gf_smp_config c = field_config(max_nVertices, nLevels, nChanels, nFeatures, nDepth, wl);
    c.first_order = form;   // 1: SMP_theta, 2 .. 4: SMP_1D, SMP_1D_ver2, SMP_1D_ver3
    return c;
}
inline gf_smp_config steerable_config(int form, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, bool wl) {
    gf_smp_config c = field_config(max_nVertices, nLevels, nChanels, nFeatures, nDepth, wl);
    c.steerable_2d = form;   // 1: SMP_2D, 2: SMP_2D_ver4, 5: SMP_2D_ver5
    return c;
}
inline gf_smp_config unrestricted_config(int form, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, bool wl) {
    gf_smp_config c = field_config(max_nVertices, nLevels, nChanels, nFeatures, nDepth, wl);
    c.unrestricted = form;   // 1: Unrestricted_SMP_1D, 2: _1D_ver2, 3: _2D
    return c;
}
// the vertex-level families: form = gf_smp_config.neighbourhood (1 NeuralFingerprint, 2 / 3 / 6 GCN_1D / _2D / _3D, 4 / 5 / 7 GRU_GCN_*)
inline gf_smp_config vertex_config(int form, int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth, int max_Radius) {
    gf_smp_config c = zero_config();
    c.nLevels = nLevels;
    c.nChanels = nHiddens;
    c.nFeatures = nFeatures;
    c.nDepth = nDepth;
    c.max_receptive_field = c.max_nVertices = max_nVertices;
    c.neighbourhood = form;
    c.max_Radius = max_Radius;
    return c;
}
inline gf_smp_config distance_config(int form, int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth, int max_Radius) {
    gf_smp_config c = vertex_config(form, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius);
    c.distance_channel = 1;
    return c;
}
inline gf_smp_config readout_config(int readout, int form, int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth, int max_Radius) {
    gf_smp_config c = vertex_config(form, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius);
    c.readout = readout;   // 1: pairs, 2: Gram
    return c;
}
inline gf_smp_config lcnn_config(int nVertices, int nFeatures, int nNeighbors, int nDepth, int nChanels1, int nChanels2, int nDense) {
    gf_smp_config c = vertex_config(0, 2, nVertices, nFeatures, nChanels1, nDepth, 0);
    c.matrix_form = 1;
    c.nNeighbors = nNeighbors;
    c.nChanels2 = nChanels2;
    c.nDense = nDense;
    return c;
}
inline gf_smp_config gcn_mw_config(int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth) {
    gf_smp_config c = vertex_config(0, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, 0);
    c.matrix_form = 2;
    return c;
}
inline gf_smp_config covariant_config(int form, int nLevels, int max_nVertices, int nFeatures, int nDepth) {
    gf_smp_config c = vertex_config(0, nLevels, max_nVertices, nFeatures, 1, nDepth, 0);
    c.covariant = form;   // 1: CGCN_1D, 2: CGCN_2D
    return c;
}

}  // namespace gfhost

// SMP_theta (GraphFlow/SMP_theta.h:31, :50): the one class of this file with a receptive-field cap, and with Adam
class SMP_theta_hip : public SMP_single_hip {
public:
    SMP_theta_hip(int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures, int nDepth, bool has_WL_ordering = true)
        : SMP_single_hip("SMP_theta_hip", config(max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering), 0, false, 0.0) {}

private:
    static gf_smp_config config(int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures, int nDepth, bool wl) {
        gf_smp_config c = gfhost::first_order_config(1, max_nVertices, nLevels, nChanels, nFeatures, nDepth, wl);
        c.max_receptive_field = max_receptive_field;
        return c;
    }
};

// The field-level regression classes share one argument list:
//   (max_nVertices, nLevels, nChanels, nFeatures, nDepth, momentum_param[, has_WL_ordering])            e.g. GraphFlow/SMP_1D.h:32, :45
// and their classifiers the same behind nClass                                                            e.g. SMP_1D_classification.h:32, :46
#define GF_FIELD_CLASS(NAME, CONFIG, FORM)                                                                                                   \
    class NAME##_hip : public SMP_single_hip {                                                                                               \
    public:                                                                                                                                  \
        NAME##_hip(int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, double momentum_param, bool has_WL_ordering = true) \
            : SMP_single_hip(#NAME "_hip", gfhost::CONFIG(FORM, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering), 0, true, \
                             momentum_param) {}                                                                                              \
    };
#define GF_FIELD_CLASSIFIER(NAME, CONFIG, FORM)                                                                                              \
    class NAME##_hip : public SMP_single_hip {                                                                                               \
    public:                                                                                                                                  \
        NAME##_hip(int nClass, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, double momentum_param,               \
                   bool has_WL_ordering = true)                                                                                              \
            : SMP_single_hip(#NAME "_hip", gfhost::CONFIG(FORM, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering), nClass, \
                             true, momentum_param) {}                                                                                        \
    };
GF_FIELD_CLASS(SMP_1D, first_order_config, 2)
GF_FIELD_CLASS(SMP_1D_ver2, first_order_config, 3)
GF_FIELD_CLASS(SMP_1D_ver3, first_order_config, 4)
GF_FIELD_CLASSIFIER(SMP_1D_classification, first_order_config, 2)
GF_FIELD_CLASSIFIER(SMP_1D_ver3_classification, first_order_config, 4)
GF_FIELD_CLASS(SMP_2D, steerable_config, 1)
GF_FIELD_CLASS(SMP_2D_ver4, steerable_config, 2)
GF_FIELD_CLASS(SMP_2D_ver5, steerable_config, 5)
GF_FIELD_CLASSIFIER(SMP_2D_classification, steerable_config, 1)
GF_FIELD_CLASSIFIER(SMP_2D_ver4_classification, steerable_config, 2)
GF_FIELD_CLASS(Unrestricted_SMP_1D, unrestricted_config, 1)
GF_FIELD_CLASS(Unrestricted_SMP_1D_ver2, unrestricted_config, 2)
GF_FIELD_CLASS(Unrestricted_SMP_2D, unrestricted_config, 3)
#undef GF_FIELD_CLASS
#undef GF_FIELD_CLASSIFIER

// NeuralFingerprint (GraphFlow/NeuralFingerprint.h:28): raw vertex features (no nDepth), the bonds as neighbourhoods (no max_Radius)
class NeuralFingerprint_hip : public SMP_single_hip {
public:
    NeuralFingerprint_hip(int nLevels, int max_nVertices, int nFeatures, int nHiddens, double momentum_param)
        : SMP_single_hip("NeuralFingerprint_hip", gfhost::vertex_config(1, nLevels, max_nVertices, nFeatures, nHiddens, 0, 0), 0, true, momentum_param) {}
};

// The vertex-level classes share one argument list:
//   (nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius, momentum_param)                    e.g. GraphFlow/GCN_1D.h:30
#define GF_VERTEX_CLASS(NAME, BASE, CONFIG)                                                                                       \
    class NAME##_hip : public BASE {                                                                                              \
    public:                                                                                                                       \
        NAME##_hip(int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth, int max_Radius, double momentum_param) \
            : BASE(#NAME "_hip", gfhost::CONFIG, momentum_param) {}                                                               \
    };
#define GF_VERTEX_ARGS nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius
class SMP_vertex_hip : public SMP_single_hip {   // (regression with Momentum: the (name, config, momentum) constructor of the two bases below)
protected:
    SMP_vertex_hip(const char *name, const gf_smp_config &cfg, double momentum_param) : SMP_single_hip(name, cfg, 0, true, momentum_param) {}
};
GF_VERTEX_CLASS(GCN_1D, SMP_vertex_hip, vertex_config(2, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_2D, SMP_vertex_hip, vertex_config(3, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_3D, SMP_vertex_hip, vertex_config(6, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GRU_GCN_1D, SMP_vertex_hip, vertex_config(4, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GRU_GCN_2D, SMP_vertex_hip, vertex_config(5, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GRU_GCN_3D, SMP_vertex_hip, vertex_config(7, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_1D_Distance, SMP_vertex_hip, distance_config(2, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_2D_Distance, SMP_vertex_hip, distance_config(3, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_3D_Distance, SMP_vertex_hip, distance_config(6, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_1D_Kernel, SMP_pairs_hip, readout_config(1, 2, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_2D_Kernel, SMP_pairs_hip, readout_config(1, 3, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCN_3D_Kernel, SMP_pairs_hip, readout_config(1, 6, GF_VERTEX_ARGS))
GF_VERTEX_CLASS(GCA_1D, SMP_gram_hip, readout_config(2, 2, GF_VERTEX_ARGS))
#undef GF_VERTEX_CLASS
#undef GF_VERTEX_ARGS

// LCNN (GraphFlow/LCNN.h:32) and GCN_MW (GCN_MW.h:30): the matrix-form baselines
class LCNN_hip : public SMP_single_hip {
public:
    LCNN_hip(int nVertices, int nFeatures, int nNeighbors, int nDepth, int nChanels1, int nChanels2, int nDense, double momentum_param)
        : SMP_single_hip("LCNN_hip", gfhost::lcnn_config(nVertices, nFeatures, nNeighbors, nDepth, nChanels1, nChanels2, nDense), 0, true, momentum_param) {}
};
class GCN_MW_hip : public SMP_single_hip {
public:
    GCN_MW_hip(int nLevels, int max_nVertices, int nFeatures, int nHiddens, int nDepth, double momentum_param)
        : SMP_single_hip("GCN_MW_hip", gfhost::gcn_mw_config(nLevels, max_nVertices, nFeatures, nHiddens, nDepth), 0, true, momentum_param) {}
};

// CGCN_1D, CGCN_2D (GraphFlow/CGCN_1D.h:30, CGCN_2D.h:30): the covariant vertex level; Feature has max_nVertices entries
class CGCN_1D_hip : public SMP_single_hip {
public:
    CGCN_1D_hip(int nLevels, int max_nVertices, int nFeatures, int nDepth, double momentum_param)
        : SMP_single_hip("CGCN_1D_hip", gfhost::covariant_config(1, nLevels, max_nVertices, nFeatures, nDepth), 0, true, momentum_param) {}
};
class CGCN_2D_hip : public SMP_single_hip {
public:
    CGCN_2D_hip(int nLevels, int max_nVertices, int nFeatures, int nDepth, double momentum_param)
        : SMP_single_hip("CGCN_2D_hip", gfhost::covariant_config(2, nLevels, max_nVertices, nFeatures, nDepth), 0, true, momentum_param) {}
};

#endif
