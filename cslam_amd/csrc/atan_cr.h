// atan_cr.h -- arctangent of a non-negative float64, rounded to nearest from a double-double evaluation.
//
// The ScanContext descriptor takes floor(theta / gap_sector) of theta = (180 / pi) * atan(y / x): a point on a sector
// edge changes bin with the last bit of the arctangent, and the device library's atan is good to a few ulp only.
// The reference's numpy calls the C library's atan, which is not correctly rounded everywhere either (glibc: the last
// bit is off for roughly one argument in a thousand), so this function is not bit-identical to the reference or to
// oracle/sc_oracle.c: it agrees with them wherever libm rounds correctly, and elsewhere wherever that bit does not move
// a point across a sector edge.  tests/golden/sc_edges_g13.npz carries the libm that recorded it; at its sector-edge
// points that libm, numpy and this function agree (tests/test_atan_cr_cpu.py checks this function against mpmath).
// C++ only (device code, and host builds for that test).  Here: z = r or 1 / r in [0, 1] (as a double-double), t = the nearest multiple of
// 1/256, atan(z) = atan(t) + atan(d) with d = (z - t) / (1 + z t), |d| <= 2^-9, atan(t) from a double-double table and
// atan(d) from its series (d in double-double, the terms from d^3 on in float64: below 2^-72 of the result).
// Table: python, mpmath at 200 bits: a = atan(i / 256); hi = float(a); lo = float(a - hi), printed with float.hex.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define ATAN_CR_FN __host__ __device__ __forceinline__
#define ATAN_CR_TABLE static __device__ const double
#else
#define ATAN_CR_FN static inline
#define ATAN_CR_TABLE static const double
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define ACR_ADD(a, b) __dadd_rn(a, b)      // never contracted into an fma
#define ACR_SUB(a, b) __dsub_rn(a, b)
#define ACR_MUL(a, b) __dmul_rn(a, b)
#define ACR_DIV(a, b) __ddiv_rn(a, b)
#else                                      // host builds of this header: compile with -ffp-contract=off
#define ACR_ADD(a, b) ((a) + (b))
#define ACR_SUB(a, b) ((a) - (b))
#define ACR_MUL(a, b) ((a) * (b))
#define ACR_DIV(a, b) ((a) / (b))
#endif

ATAN_CR_TABLE ATAN_CR_TAB[257][2] = {      // atan(i / 256) = [i][0] + [i][1]
    {0x0.0p+0, 0x0.0p+0},
    {0x1.ffff5555bbbb7p-9, 0x1.4bb12afb6b6d5p-64},
    {0x1.fffd555bbba97p-8, 0x1.68062351fbbe6p-63},
    {0x1.7ffb80184c30ap-7, -0x1.725017508234bp-61},
    {0x1.fff555bbb729bp-7, -0x1.220c39d4dff50p-61},
    {0x1.3ff595f18a700p-6, -0x1.213eac36cfb2cp-60},
    {0x1.7fee0184a5c36p-6, -0x1.43189fc0a354bp-60},
    {0x1.bfe36df291712p-6, -0x1.e1bec7756100ep-61},
    {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},
    {0x1.1fe1a5c2ec497p-5, 0x1.886091e8fc4cbp-59},
    {0x1.3fd65f169c9d9p-5, 0x1.7230a716461b5p-61},
    {0x1.5fc89a5fa3b2dp-5, 0x1.2bb73bf4e7f99p-59},
    {0x1.7fb818430da2ap-5, -0x1.86ef8f794f105p-63},
    {0x1.9fa49986984dfp-5, 0x1.322907af0abc2p-59},
    {0x1.bf8ddf139c444p-5, -0x1.89fe34b2a7fa8p-59},
    {0x1.df73a9f9f1882p-5, -0x1.251b5c410bcb4p-62},
    {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},
    {0x1.0f99ea71d52a7p-4, -0x1.2069feec3624fp-61},
    {0x1.1f86dbf082d59p-4, -0x1.095dc7732ef81p-59},
    {0x1.2f719318a4a9ap-4, 0x1.3fd1779b9801fp-63},
    {0x1.3f59f0e7c559dp-4, 0x1.ac4ce285df847p-58},
    {0x1.4f3fd677292fbp-4, 0x1.008d36264979ep-59},
    {0x1.5f2324fd2d7b2p-4, 0x1.8a8da4401318ep-58},
    {0x1.6f03bdcea4b0dp-4, -0x1.3f00e512fa17dp-60},
    {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},
    {0x1.8ebc54478fb28p-4, 0x1.732880cad24ccp-59},
    {0x1.9e94153cfdcf1p-4, 0x1.a332e1d69c47ep-58},
    {0x1.ae68a71c722b8p-4, 0x1.c014e6910b9dbp-59},
    {0x1.be39ebe6f07c3p-4, 0x1.f7b8f29a05987p-58},
    {0x1.ce07c5c3cca32p-4, 0x1.138e6425918a7p-59},
    {0x1.ddd21701eba6ep-4, 0x1.94effcd76fe58p-58},
    {0x1.ed98c2190043bp-4, -0x1.3a598592c7b13p-61},
    {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},
    {0x1.068d584212b3ep-3, -0x1.9e2d283019bfdp-57},
    {0x1.0e6adccf40882p-3, -0x1.d71a31bb98d0dp-57},
    {0x1.1646541060850p-3, 0x1.6bcee8ae7ea92p-57},
    {0x1.1e1fafb043727p-3, -0x1.b485914dacf8cp-59},
    {0x1.25f6e171a535cp-3, 0x1.7c6d7bde1a310p-57},
    {0x1.2dcbdb2fba1ffp-3, 0x1.8f28705561534p-58},
    {0x1.359e8edeb99a4p-3, -0x1.a5fd74e4604c6p-57},
    {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},
    {0x1.453cec6092a9ep-3, 0x1.1f653b3a5a78bp-57},
    {0x1.4d087a9da4f17p-3, 0x1.1f323f1adf158p-57},
    {0x1.54d18ba11570ap-3, 0x1.18282f2884073p-57},
    {0x1.5c9811e3ec26ap-3, -0x1.054ab2c010f3dp-58},
    {0x1.645bfffb3aa74p-3, -0x1.f536b677c2cb4p-60},
    {0x1.6c1d4898933d9p-3, -0x1.2954a7603c427p-58},
    {0x1.73dbde8a7d202p-3, -0x1.5ad0f6d4a665dp-58},
    {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},
    {0x1.8350be398ebc8p-3, -0x1.5a91332b9c90dp-58},
    {0x1.8b06ee2879c29p-3, -0x1.118cd30308c4fp-57},
    {0x1.92ba37d050272p-3, -0x1.0d3ded0ff4764p-57},
    {0x1.9a6a8e96c8626p-3, 0x1.cf601e7b4348ep-59},
    {0x1.a217e601081a6p-3, -0x1.0def8a60af374p-57},
    {0x1.a9c231b403279p-3, 0x1.0e8bbe89cca85p-57},
    {0x1.b1696574d780cp-3, -0x1.85ab8fc15a673p-58},
    {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},
    {0x1.c0ae54d768467p-3, -0x1.04cdbf55f26dcp-57},
    {0x1.c84bf8a742e6ep-3, -0x1.95bdd0682ea26p-58},
    {0x1.cfe654e1d5395p-3, 0x1.47b9a3f71eafbp-57},
    {0x1.d77d5df205736p-3, 0x1.c648d1534597ep-57},
    {0x1.df110864c9d9ep-3, -0x1.5818b53bf4781p-60},
    {0x1.e6a148e96ec4dp-3, 0x1.866b22029f765p-57},
    {0x1.ee2e1451d980dp-3, -0x1.9a7708c46ba91p-58},
    {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
    {0x1.fd3d1fc40dbe4p-3, 0x1.37146f3a1c5eap-59},
    {0x1.025fa510665b6p-2, -0x1.672df6832fa48p-56},
    {0x1.061eea03d6291p-2, -0x1.5f760db154301p-59},
    {0x1.09dc597d86362p-2, 0x1.62e47390cb865p-56},
    {0x1.0d97ee509acb3p-2, 0x1.47c317bd5a3ebp-56},
    {0x1.1151a362431cap-2, -0x1.4dc8dc9077b9fp-56},
    {0x1.150973a9ce547p-2, -0x1.796ba7f9ca328p-56},
    {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},
    {0x1.1c735212dd884p-2, -0x1.7d9ac78cb2f2ep-57},
    {0x1.2025567e47c96p-2, -0x1.1832328f4290ep-57},
    {0x1.23d562b381042p-2, -0x1.c531716200088p-58},
    {0x1.278372057ef46p-2, -0x1.077cdd36dfc81p-56},
    {0x1.2b2f7fd9b5fe2p-2, 0x1.423cfc1c2d443p-61},
    {0x1.2ed987a823cfep-2, 0x1.b91258ea012cap-57},
    {0x1.328184fb58952p-2, -0x1.a95f0a9939f2fp-56},
    {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},
    {0x1.39cb4eb76157cp-2, -0x1.2f4da5a214713p-56},
    {0x1.3d6d129271134p-2, 0x1.137ca41cc958ap-56},
    {0x1.410cbad6c7d33p-2, -0x1.b0c8bae13b512p-56},
    {0x1.44aa436c2af0ap-2, -0x1.5d5e43c55b3bap-56},
    {0x1.4845a84d0c21bp-2, 0x1.1e28a7563c6a6p-56},
    {0x1.4bdee586890e7p-2, -0x1.e4dc77c22a757p-57},
    {0x1.4f75f73869979p-2, -0x1.95a1cf7ff1108p-58},
    {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},
    {0x1.569d88e1b4cd8p-2, -0x1.fec61e713cfe2p-57},
    {0x1.5a2e0175e0f4ep-2, 0x1.13b7a8f82e457p-56},
    {0x1.5dbc3fbbe768dp-2, 0x1.ea0ec1b76f7dap-57},
    {0x1.614840309cfe2p-2, -0x1.a725715711f00p-56},
    {0x1.64d1ff635c1c6p-2, -0x1.fa403e7c0fdbep-56},
    {0x1.685979f5fa6fep-2, -0x1.257814d1ada9cp-59},
    {0x1.6bdeac9cbd76dp-2, -0x1.a5c563e6de828p-58},
    {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},
    {0x1.72e22d53aa2aap-2, -0x1.d9c934e79f27cp-56},
    {0x1.7660752817502p-2, -0x1.dd11791cc7600p-59},
    {0x1.79dc6899118d1p-2, 0x1.b7413a0ef606dp-61},
    {0x1.7d5604b63b3f7p-2, 0x1.69c885c2b249ap-56},
    {0x1.80cd46a14b1d1p-2, -0x1.e79f99684fa19p-56},
    {0x1.84422b8df95d7p-2, 0x1.d76a0299b41b6p-56},
    {0x1.87b4b0c1ebedcp-2, -0x1.6dcfaa2fa470fp-56},
    {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},
    {0x1.8e92916f5cde8p-2, 0x1.4c0a7e12bfafbp-56},
    {0x1.91fde7cd0c662p-2, 0x1.1074188054b53p-56},
    {0x1.9566d43a34907p-2, 0x1.9b01537e0af2bp-57},
    {0x1.98cd5454d6b18p-2, 0x1.9e6c988fd0a77p-56},
    {0x1.9c3165cc58107p-2, 0x1.b669602250cfbp-59},
    {0x1.9f93066168002p-2, -0x1.c827047c9439ap-56},
    {0x1.a2f233e5e530bp-2, 0x1.814d5f797086bp-58},
    {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},
    {0x1.a9a92d59e98cfp-2, 0x1.2e42dff75d817p-59},
    {0x1.ad00f5422058bp-2, 0x1.fc4c33891d2e8p-56},
    {0x1.b056420ae9344p-2, -0x1.9313946363455p-56},
    {0x1.b3a911da65c6cp-2, 0x1.ae187b1ca5040p-56},
    {0x1.b6f962e737efcp-2, -0x1.ca53464981e71p-58},
    {0x1.ba473378624a5p-2, 0x1.519a1b46e4affp-56},
    {0x1.bd9281e528192p-2, -0x1.4b15439af6b66p-56},
    {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},
    {0x1.c42191ff11eb7p-2, -0x1.b17df434b3eeep-56},
    {0x1.c76550aad71f9p-2, -0x1.74b8bff7043e4p-56},
    {0x1.caa6872f3631bp-2, 0x1.9506781636f48p-61},
    {0x1.cde53432c1351p-2, -0x1.a2cfa4418f1adp-56},
    {0x1.d121566b7f2adp-2, 0x1.be67835886c30p-56},
    {0x1.d45aec9ec862bp-2, 0x1.89421163ef92dp-57},
    {0x1.d791f5a1226f5p-2, -0x1.4017ea5b64a76p-57},
    {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},
    {0x1.ddf85bb026974p-2, 0x1.43bbb0c0a1226p-57},
    {0x1.e127b6b0744b0p-2, -0x1.2b0986398d4abp-58},
    {0x1.e4548066cf51ap-2, 0x1.3a3aa12ce98f2p-59},
    {0x1.e77eb7f175a34p-2, 0x1.0e53dc1bf3435p-56},
    {0x1.eaa65c7cf28c4p-2, 0x1.2fb2ceca3bf05p-57},
    {0x1.edcb6d43f8435p-2, -0x1.fc976330884e4p-58},
    {0x1.f0ede98f393d0p-2, -0x1.2f40a87cb1894p-56},
    {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},
    {0x1.f72b221a4e495p-2, 0x1.489c20f7eb740p-58},
    {0x1.fa45dd3029259p-2, -0x1.ca563dc28d8b5p-56},
    {0x1.fd5e0175fdf83p-2, 0x1.3a87b1ec49b15p-57},
    {0x1.0039c73c1a40cp-1, -0x1.b32c949c9d593p-55},
    {0x1.01c341e82422dp-1, 0x1.3db44fcca90eep-55},
    {0x1.034b709250488p-1, 0x1.8f9b38d855410p-56},
    {0x1.04d25314342e6p-1, -0x1.1c8636442c767p-55},
    {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},
    {0x1.07dc3324e9b38p-1, 0x1.b70c9e04450acp-56},
    {0x1.095f30861a590p-1, -0x1.121b20a15a9f3p-56},
    {0x1.0ae0e1639866cp-1, 0x1.075abf2de445ap-56},
    {0x1.0c6145b5b43dap-1, 0x1.974fa13b5404fp-58},
    {0x1.0de05d7aa6f7dp-1, -0x1.83684b1c529abp-56},
    {0x1.0f5e28b67e295p-1, 0x1.311b17ec990d0p-65},
    {0x1.10daa77307a0dp-1, 0x1.69c33d44c7b05p-55},
    {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},
    {0x1.13cfbfb1b056ep-1, 0x1.3110e6fc3ed38p-55},
    {0x1.154859637646ap-1, -0x1.4ba7c548bf3c3p-55},
    {0x1.16bfa6f5137e1p-1, 0x1.9606fe141bd35p-56},
    {0x1.1835a88be7c13p-1, 0x1.c621cec00c301p-55},
    {0x1.19aa5e5299f9ap-1, -0x1.a606c2c58f835p-55},
    {0x1.1b1dc87904285p-1, -0x1.21e8c8aef8f29p-57},
    {0x1.1c8fe7341f64fp-1, 0x1.28bbc9d5e792ap-56},
    {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
    {0x1.1f7043557138ap-1, 0x1.6c659f6d7dd47p-56},
    {0x1.20de813e823b2p-1, -0x1.791d753ebb744p-55},
    {0x1.224b74c1d192ap-1, 0x1.d6d3df88a60c4p-55},
    {0x1.23b71e2cc9e6ap-1, 0x1.c421c9f38224ep-57},
    {0x1.25217dd17e501p-1, 0x1.56aa88c1b679cp-55},
    {0x1.268a940696da6p-1, 0x1.d1348a04c73ccp-58},
    {0x1.27f261273d1b3p-1, 0x1.43bf36151dd9fp-55},
    {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},
    {0x1.2abe21aded073p-1, 0x1.c28c001ad022ep-55},
    {0x1.2c2215e024466p-1, -0x1.4b810da3a4be1p-59},
    {0x1.2d84c2961e48cp-1, -0x1.f25420a36e506p-56},
    {0x1.2ee628406cbcap-1, 0x1.c5d5e9ff0cf8dp-55},
    {0x1.30464753b090bp-1, -0x1.3e71261da18f3p-56},
    {0x1.31a52048874bep-1, 0x1.40cab87a7ac24p-55},
    {0x1.3302b39b78856p-1, 0x1.5dd2ed87ba82bp-55},
    {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},
    {0x1.35ba0b60ecccep-1, 0x1.e3ba19b9368b9p-55},
    {0x1.3713d0df6c504p-1, -0x1.4f789e031606dp-58},
    {0x1.386c52d3db11fp-1, -0x1.b78e1cbebe6a0p-55},
    {0x1.39c391cd4171ap-1, -0x1.2304331d8bf46p-55},
    {0x1.3b198e5e2564bp-1, -0x1.2f9221f0752acp-56},
    {0x1.3c6e491c78dc5p-1, -0x1.e145094fd0ba7p-55},
    {0x1.3dc1c2a188504p-1, 0x1.2ce6370f4e971p-55},
    {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},
    {0x1.4064f47569f49p-1, -0x1.aad88f91bf2b2p-55},
    {0x1.41b4ae06fea41p-1, 0x1.3d60a53277652p-57},
    {0x1.430328e4b26d6p-1, -0x1.131591070b99fp-55},
    {0x1.445065b795b56p-1, -0x1.f76d0163f79c8p-56},
    {0x1.459c652badc7fp-1, 0x1.199698e8e135cp-55},
    {0x1.46e727efe4716p-1, -0x1.39b9b1b844cc9p-57},
    {0x1.4830aeb5f7bfep-1, -0x1.a265666764a73p-58},
    {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},
    {0x1.4ac00b1c71762p-1, 0x1.b20e72382b900p-55},
    {0x1.4c05e22de94e5p-1, -0x1.c0ac1f09f2edfp-55},
    {0x1.4d4a8023414e8p-1, 0x1.e3a891daa88b0p-57},
    {0x1.4e8de5bb6ec04p-1, 0x1.4a33dbeb3796cp-55},
    {0x1.4fd013b7dd17ep-1, 0x1.d513f3e7c24b5p-56},
    {0x1.51110adc5ed81p-1, 0x1.23dcd6832a63ep-56},
    {0x1.5250cbef1e9fbp-1, -0x1.539b7a3228870p-58},
    {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},
    {0x1.54ccaf0362c8fp-1, 0x1.8a3247f8f43c1p-55},
    {0x1.5608d29c70c34p-1, 0x1.9939cf0de8088p-55},
    {0x1.5743c352b33bap-1, -0x1.ea00d34c87ea6p-55},
    {0x1.587d81f732fbbp-1, -0x1.5e5c9d8c5a950p-56},
    {0x1.59b60f5cfab9ep-1, -0x1.1b04c41026bc5p-55},
    {0x1.5aed6c5909517p-1, 0x1.7312f714a9436p-55},
    {0x1.5c2399c244261p-1, -0x1.31bd4e9e56b35p-55},
    {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},
    {0x1.5e8c6941043d0p-1, -0x1.0bf75be451e70p-56},
    {0x1.5fbf0d0d5cc4ap-1, -0x1.b4cfd000b7158p-58},
    {0x1.60f084b46e05fp-1, -0x1.dbb8699945193p-55},
    {0x1.6220d115d7b8ep-1, -0x1.2b785350ee8c1p-57},
    {0x1.634ff312d1f3bp-1, 0x1.9d2f315f2b598p-55},
    {0x1.647deb8e20b90p-1, -0x1.eca04023a51cfp-58},
    {0x1.65aabb6c07b03p-1, -0x1.7939b3af32729p-57},
    {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},
    {0x1.6800e4e7e2858p-1, -0x1.8ea6a1b3e90f0p-58},
    {0x1.692a40556fb6ap-1, 0x1.d94b95a8ea2ccp-55},
    {0x1.6a5276c4b0576p-1, -0x1.f6b659c46a69ep-55},
    {0x1.6b798920b3d99p-1, -0x1.a80386188c50ep-55},
    {0x1.6c9f7855c3198p-1, 0x1.c09de29bd280dp-56},
    {0x1.6dc44551553afp-1, -0x1.bf8863573828ep-58},
    {0x1.6ee7f10204aefp-1, 0x1.692eea3066272p-55},
    {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},
    {0x1.712be84295198p-1, 0x1.5cd90337d8881p-55},
    {0x1.724c35b4fae7bp-1, 0x1.948b32db3499bp-58},
    {0x1.736b65a172dffp-1, 0x1.775fd06a892d1p-56},
    {0x1.748978fba8e0fp-1, 0x1.7b2a6165884a1p-59},
    {0x1.75a670b82d8d8p-1, 0x1.ee4ac4c729087p-55},
    {0x1.76c24dcc6c6c0p-1, 0x1.1952551adc83dp-55},
    {0x1.77dd112ea22c7p-1, 0x1.732608fc10d3dp-55},
    {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},
    {0x1.7a0f4eb9c19a2p-1, 0x1.13c67cd815f57p-57},
    {0x1.7b26cad2e50fep-1, -0x1.ce80df30411fbp-55},
    {0x1.7c3d311a6092bp-1, 0x1.bb3cb2d303288p-55},
    {0x1.7d528289fa093p-1, 0x1.560821e2f3aa9p-55},
    {0x1.7e66c01c114fep-1, -0x1.c82b88b760b8dp-55},
    {0x1.7f79eacb97898p-1, 0x1.fd5ca80ead221p-55},
    {0x1.808c03940694bp-1, -0x1.00f327715f6a5p-55},
    {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},
    {0x1.82ad036000005p-1, 0x1.4592fce924d24p-56},
    {0x1.83bbec5cdee22p-1, 0x1.3107104ffc6c3p-57},
    {0x1.84c9c7653f7ebp-1, -0x1.83611fe0a3e8fp-60},
    {0x1.85d69576cc2c5p-1, 0x1.6b66e7fc8b8c3p-57},
    {0x1.86e2578f87ae5p-1, 0x1.022b1375cfe34p-55},
    {0x1.87ed0eadc5a2ap-1, 0x1.0af5ad957f4bcp-56},
    {0x1.88f6bbd023119p-1, -0x1.32d1d25aba660p-58},
    {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},
    {0x1.8b06fc1cf3dffp-1, -0x1.0fb312656db6dp-55},
    {0x1.8c0d9145cf49dp-1, 0x1.bea4076dc4333p-55},
    {0x1.8d13206f8c4cbp-1, -0x1.b018cbaa89a8bp-56},
    {0x1.8e17aa99cc05ep-1, -0x1.ec182ab042f61p-56},
    {0x1.8f1b30c44f167p-1, 0x1.dd1cab93933fdp-57},
    {0x1.901db3eeef187p-1, 0x1.68665e5603c8fp-55},
    {0x1.911f35199833bp-1, 0x1.3ae8a0edbf522p-57},
    {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55},
};

// s + e = a + b exactly
ATAN_CR_FN double acr_two_sum(double a, double b, double *e) {
    const double s = ACR_ADD(a, b), bb = ACR_SUB(s, a);
    *e = ACR_ADD(ACR_SUB(a, ACR_SUB(s, bb)), ACR_SUB(b, bb));
    return s;
}

ATAN_CR_FN double atan_cr(double r) {      // r >= 0 (NaN gives NaN)
    const double PIH = 0x1.921fb54442d18p+0, PIL = 0x1.1a62633145c07p-54;       // pi / 2
    if (r != r) return r;
    if (r < 0x1p-27) return r;             // r - r^3 / 3 rounds to r
    if (r > 0x1p55) return PIH;            // pi / 2 - 1 / r rounds to pi / 2
    const bool inv = r > 1.0;
    double zh = r, zl = 0.0;
    if (inv) {
        zh = ACR_DIV(1.0, r);
        zl = ACR_DIV(fma(-zh, r, 1.0), r);
    }
    const int i = (int)rint(ACR_MUL(zh, 256.0));
    const double t = (double)i * 0x1p-8;
    // d = (z - t) / (1 + z t); zh - t is exact (Sterbenz)
    double nl, dl, e;
    const double nh = acr_two_sum(ACR_SUB(zh, t), zl, &nl);
    const double ph = ACR_MUL(zh, t), pl = fma(zh, t, -ph);
    const double dh = acr_two_sum(1.0, ph, &e);
    dl = ACR_ADD(ACR_ADD(e, pl), ACR_MUL(zl, t));
    const double qh = ACR_DIV(nh, dh);
    const double rem = ACR_SUB(ACR_ADD(fma(-qh, dh, nh), nl), ACR_MUL(qh, dl));
    const double ql = ACR_DIV(rem, dh);
    // atan(d) - d = -d^3/3 + d^5/5 - d^7/7 + d^9/9, |d| <= 2^-9
    const double d2 = ACR_MUL(qh, qh);
    double p = fma(d2, 1.0 / 9.0, -1.0 / 7.0);
    p = fma(d2, p, 1.0 / 5.0);
    p = fma(d2, p, -1.0 / 3.0);
    double tail = ACR_MUL(ACR_MUL(qh, d2), p);
    tail = ACR_SUB(tail, ACR_MUL(d2, ql));
    double ul;
    const double uh = acr_two_sum(ATAN_CR_TAB[i][0], qh, &ul);
    ul = ACR_ADD(ul, ACR_ADD(ACR_ADD(ATAN_CR_TAB[i][1], ql), tail));
    if (!inv) return ACR_ADD(uh, ul);
    double vl;
    const double vh = acr_two_sum(PIH, -uh, &vl);
    return ACR_ADD(vh, ACR_ADD(vl, ACR_SUB(PIL, ul)));
}
