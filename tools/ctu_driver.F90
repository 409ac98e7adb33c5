! Driver of tools/make_golden_ctu.py: calls the reference's corner-transport path -- PROPDOT (with GRADI), CTUWINI, CTUWDRV (with CTUW) and PROPAGS2 --
! on the cases of a stream file and writes what they return.  It is built by oracle/ref_build.py::build_driver: the routines and the modules they use are
! the reference's own files, compiled unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90.  One module is the driver's own: OML_MOD
! (another package, fiat), of which CTUWDRV calls one function; it answers 1 thread, so that CTUWDRV makes one block of all points.
! Around the calls the program does what CTUWUPDT and PROPAG_WAM do around theirs, in the driver's own words:
!   the selectors KPM, MPM, JXO, JYO, KCR                              ctuwupdt.F90:93-161
!   CTUWINI once, CTUWDRV once, or twice with a split                  ctuwupdt.F90:207-254
!   the flags LLW* of the general PROPAGS2 branch (IREFRA 2, 3)        ctuwupdt.F90:263-337
!   PROPAGS2 on all frequencies, then the second sub-step of the fast  propag_wam.F90:239-313
!   waves (NSTEP_LF = 2: DELPRO_LF = IDELPRO / 2)
! LCFLFAIL and CURMASK are locals of CTUWDRV and CTUW.  To have them the program makes, before each CTUWDRV call, the CTUW calls CTUWDRV is about to make
! (ICALL = 1 on all points; ICALL = 2 where LLCFLCUROFF, currents and a failing point ask for it, ctuwdrv.F90:93-122) with a flag array of its own, keeps
! the weights, and requires after CTUWDRV that every weight is the same number: what is recorded is what CTUWDRV left.  CURMASK is the mask CTUW derives
! from the flags of the first call (ctuw.F90:114-128).  A case whose flags survive the second call is refused: CTUWDRV aborts there.
! Input  (stream, little endian): N, NANG, NFRE_RED, NGY (int32); FR(NFRE_RED), SINTH(NANG), COSTH(NANG), then DELTH, R, ZPI, PI, XDELLA, DELPHI (real64);
!        ZDELLO(NGY), DELLAM(NGY), SINPH(NGY), COSPH(NGY) (real64); KXLT(N), KLON(N,2), KLAT(N,2,2), KCOR(N,4,2) (int32, 1-based, the land row is N+1);
!        WLAT(N,2), WCOR(N,4), COSPHM1(N+1) (real64); then cases, each led by an int32 1 (0 ends the file):
!          IREFRA, IDELPRO, LOBS, LCUROFF, IFRELFMAX (int32); DELPRO_LF (real64); DEPTH, U, V (N+1 each); CGROUP, OMOSNH2KD, WAVNUM (N+1,NFRE_RED each);
!          with LOBS /= 0 OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2), OBSCOR(N,NFRE_RED,4); F1(N+1,NANG,NFRE_RED)
!        Every real is representable in the working precision.
! Output (stream, real64: the working-precision results, widened): CIRC, FRATIO (the reference's PARAMETERs); per case F3(N,NANG,NFRE_RED), THDD(N,NANG),
!        THDC(N,NANG), SDOT(N,NANG,NFRE_RED), FAIL1(N,2), CURMASK(N,2), FAIL(N,2) (per CTUWDRV call; the second column of a case without a split is
!        0, 1, 0), WLAT(N,2), WCOR(N,4) as CTUWINI left them, SUMWN(N,NANG,NFRE_RED), WLONN(..,2), WLATN(..,2,2), WCORN(..,4,2), WKPMN(..,-1:1), WMPMN(..,-1:1)
MODULE OML_MOD
  IMPLICIT NONE
CONTAINS
  INTEGER FUNCTION OML_GET_MAX_THREADS()
    OML_GET_MAX_THREADS = 1
  END FUNCTION OML_GET_MAX_THREADS
END MODULE OML_MOD

PROGRAM CTU_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWDRVTYPE, ONLY : WVGRIDGLO
  USE EC_LUN, ONLY : NULERR
  USE YOWCURR, ONLY : LLCFLCUROFF
  USE YOWFRED, ONLY : FR, DELTH, FRATIO, COSTH, SINTH
  USE YOWGRID, ONLY : DELPHI, DELLAM, SINPH, COSPH
  USE YOWMAP, ONLY : IRGG, IPER, NIBLO, NGY, XDELLA, ZDELLO, AMOWEP, AMOSOP
  USE YOWMPP, ONLY : IRANK
  USE YOWPARAM, ONLY : NANG, NFRE, NFRE_RED
  USE YOWPCONS, ONLY : PI, ZPI, R, CIRC
  USE YOWREFD, ONLY : THDD, THDC, SDOT
  USE YOWSTAT, ONLY : IDELPRO, ICASE, IREFRA
  USE YOWTEST, ONLY : IU06
  USE YOWUBUF, ONLY : KLAT, KLON, KCOR, WLAT, WCOR, SUMWN, WLATN, WLONN, WCORN, WKPMN, WMPMN, OBSLAT, OBSLON, OBSCOR, KPM, MPM, JXO, JYO, KCR, &
 &                    LLWLATN, LLWLONN, LLWCORN, LLWKPMN, LLWMPMN
  IMPLICIT NONE
#include "propdot.intfb.h"
#include "ctuwini.intfb.h"
#include "ctuw.intfb.h"
#include "ctuwdrv.intfb.h"
#include "propags2.intfb.h"
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER(KIND=JWIM) :: N, OP, LOBS, LCUROFF, IFRELFMAX, K, M, IC, ICL, ICR, IS, NCALLS, MS(2), ME(2)
  TYPE(WVGRIDGLO) :: BLK2GLO
  INTEGER(KIND=JWIM), ALLOCATABLE, TARGET :: KXLT(:), IXLG(:)
  REAL(KIND=R8) :: S(6), D8
  REAL(KIND=R8), ALLOCATABLE :: A8(:), G8(:), W8(:,:), C8(:,:), P8(:,:), E8(:,:,:), O8(:,:,:), F8(:,:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: F1(:,:,:), F3(:,:,:), P(:,:), E(:,:,:), COSPHM1(:), WLATM1(:,:), WCORM1(:,:), DP(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: T1(:,:,:), T2(:,:,:,:), T3(:,:,:,:,:), T4(:,:,:,:,:), T5(:,:,:,:), T6(:,:,:,:)
  REAL(KIND=JWRB) :: DELPRO_LF, DT(2)
  REAL(KIND=R8), ALLOCATABLE :: FAIL1(:,:), CURMASK(:,:), FAIL(:,:)
  LOGICAL, ALLOCATABLE :: LF1(:), LF2(:)
  LOGICAL :: CUR
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  IU06 = 13      ! CTUW's report of every number out of range: not kept
  OPEN(IU06, STATUS='SCRATCH')
  OPEN(NULERR, STATUS='SCRATCH')      ! the same report, one line per number, on the error unit
  IRANK = 1
  READ(11) N, NANG, NFRE_RED, NGY
  NFRE = NFRE_RED
  NIBLO = N
  ICASE = 1
  IRGG = 1
  IPER = 1
  AMOWEP = 0.0_JWRB
  AMOSOP = -90.0_JWRB
  ALLOCATE(FR(NFRE_RED), SINTH(NANG), COSTH(NANG), A8(NFRE_RED))
  READ(11) A8
  FR = REAL(A8, JWRB)
  DEALLOCATE(A8)
  ALLOCATE(A8(NANG))
  READ(11) A8
  SINTH = REAL(A8, JWRB)
  READ(11) A8
  COSTH = REAL(A8, JWRB)
  READ(11) S
  DELTH = REAL(S(1), JWRB)
  R = REAL(S(2), JWRB)
  ZPI = REAL(S(3), JWRB)
  PI = REAL(S(4), JWRB)
  XDELLA = REAL(S(5), JWRB)
  DELPHI = REAL(S(6), JWRB)
  ALLOCATE(ZDELLO(NGY), DELLAM(NGY), SINPH(NGY), COSPH(NGY), G8(NGY))
  READ(11) G8
  ZDELLO = REAL(G8, JWRB)
  READ(11) G8
  DELLAM = REAL(G8, JWRB)
  READ(11) G8
  SINPH = REAL(G8, JWRB)
  READ(11) G8
  COSPH = REAL(G8, JWRB)
  ALLOCATE(KXLT(N), IXLG(N), KLON(N,2), KLAT(N,2,2), KCOR(N,4,2), WLAT(N,2), WCOR(N,4), W8(N,2), C8(N,4), COSPHM1(N+1))
  READ(11) KXLT, KLON, KLAT, KCOR
  IXLG = 1      ! read by CTUW's report only
  BLK2GLO%KXLT => KXLT
  BLK2GLO%IXLG => IXLG
  DEALLOCATE(A8)
  ALLOCATE(A8(N+1))
  READ(11) W8, C8, A8
  COSPHM1 = REAL(A8, JWRB)
  ALLOCATE(OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2), OBSCOR(N,NFRE_RED,4), O8(N,NFRE_RED,8))
  ALLOCATE(P8(N+1,3), P(N+1,3), E8(N+1,NFRE_RED,3), E(N+1,NFRE_RED,3), F8(N+1,NANG,NFRE_RED), F1(N+1,NANG,NFRE_RED), F3(N+1,NANG,NFRE_RED))
  ALLOCATE(THDD(N,NANG), THDC(N,NANG), SDOT(N,NANG,NFRE_RED), WLATM1(N,2), WCORM1(N,4), DP(N,2), LF1(N), LF2(N), FAIL1(N,2), CURMASK(N,2), FAIL(N,2))
  ALLOCATE(SUMWN(N,NANG,NFRE_RED), WLONN(N,NANG,NFRE_RED,2), WLATN(N,NANG,NFRE_RED,2,2), WCORN(N,NANG,NFRE_RED,4,2), WKPMN(N,NANG,NFRE_RED,-1:1), &
 &         WMPMN(N,NANG,NFRE_RED,-1:1))
  ALLOCATE(T1(N,NANG,NFRE_RED), T2(N,NANG,NFRE_RED,2), T3(N,NANG,NFRE_RED,2,2), T4(N,NANG,NFRE_RED,4,2), T5(N,NANG,NFRE_RED,-1:1), T6(N,NANG,NFRE_RED,-1:1))
  ALLOCATE(LLWLATN(NANG,NFRE_RED,2,2), LLWLONN(NANG,NFRE_RED,2), LLWCORN(NANG,NFRE_RED,4,2), LLWKPMN(NANG,NFRE_RED,-1:1), LLWMPMN(NANG,NFRE_RED,-1:1))
  CALL SELECTORS
  WRITE(12) REAL(CIRC, R8), REAL(FRATIO, R8)
  DO
    READ(11) OP
    IF (OP == 0) EXIT
    READ(11) IREFRA, IDELPRO, LOBS, LCUROFF, IFRELFMAX, D8
    DELPRO_LF = REAL(D8, JWRB)
    LLCFLCUROFF = LCUROFF /= 0
    CUR = IREFRA == 2 .OR. IREFRA == 3
    READ(11) P8, E8
    P = REAL(P8, JWRB)
    E = REAL(E8, JWRB)
    OBSLAT = 1.0_JWRB
    OBSLON = 1.0_JWRB
    OBSCOR = 1.0_JWRB
    IF (LOBS /= 0) THEN
      READ(11) O8
      OBSLAT = REAL(O8(:,:,1:2), JWRB)
      OBSLON = REAL(O8(:,:,3:4), JWRB)
      OBSCOR = REAL(O8(:,:,5:8), JWRB)
    ENDIF
    READ(11) F8
    F1 = REAL(F8, JWRB)
    F3 = 0.0_JWRB
    WLAT = REAL(W8, JWRB)      ! CTUWINI snaps them next to land: every case starts from the grid's
    WCOR = REAL(C8, JWRB)
    THDD = 0.0_JWRB
    THDC = 0.0_JWRB
    SDOT = 0.0_JWRB
    SUMWN = 0.0_JWRB
    WKPMN = 0.0_JWRB
    WMPMN = 0.0_JWRB
    ! the dot terms (propag_wam.F90:175-212)
    IF (IREFRA /= 0) THEN
      CALL PROPDOT(1_JWIM, N, 1_JWIM, N, BLK2GLO, E(:,:,3), E(:,:,1), E(:,:,2), COSPHM1, P(:,1), P(:,2), P(:,3), THDC, THDD, SDOT)
    ENDIF
    ! the weights (ctuwupdt.F90:207-254)
    CALL CTUWINI(1_JWIM, N, 1_JWIM, N, BLK2GLO, COSPHM1, WLATM1, WCORM1, DP)
    IF (IFRELFMAX <= 0) THEN
      NCALLS = 1
      MS(1) = 1
      ME(1) = NFRE_RED
      DT(1) = REAL(IDELPRO, JWRB)
    ELSE
      NCALLS = MERGE(2, 1, IFRELFMAX < NFRE_RED)
      MS = [1, IFRELFMAX + 1]
      ME = [IFRELFMAX, NFRE_RED]
      DT = [DELPRO_LF, REAL(IDELPRO, JWRB)]
    ENDIF
    FAIL1 = 0.0_R8
    CURMASK = 1.0_R8
    FAIL = 0.0_R8
    DO IS = 1, NCALLS
      CALL CTUW(DT(IS), MS(IS), ME(IS), 1_JWIM, N, 1_JWIM, N, LF1, 1_JWIM, BLK2GLO, WLATM1, WCORM1, DP, E(:,:,1), E(:,:,2), COSPHM1, P(:,1), P(:,2), P(:,3))
      LF2 = LF1
      IF (LLCFLCUROFF .AND. CUR .AND. ANY(LF1)) THEN
        CALL CTUW(DT(IS), MS(IS), ME(IS), 1_JWIM, N, 1_JWIM, N, LF2, 2_JWIM, BLK2GLO, WLATM1, WCORM1, DP, E(:,:,1), E(:,:,2), COSPHM1, P(:,1), P(:,2), &
 &                P(:,3))
        CURMASK(:,IS) = MERGE(0.0_R8, 1.0_R8, LF1)
      ENDIF
      FAIL1(:,IS) = MERGE(1.0_R8, 0.0_R8, LF1)
      FAIL(:,IS) = MERGE(1.0_R8, 0.0_R8, LF2)
      IF (ANY(LF2)) ERROR STOP 'CTUWDRV ABORTS ON THIS CASE'
      T1 = SUMWN
      T2 = WLONN
      T3 = WLATN
      T4 = WCORN
      T5 = WKPMN
      T6 = WMPMN
      CALL CTUWDRV(DT(IS), MS(IS), ME(IS), 1_JWIM, N, 1_JWIM, N, BLK2GLO, WLATM1, WCORM1, DP, E(:,:,1), E(:,:,2), COSPHM1, P(:,1), P(:,2), P(:,3))
      IF (ANY(T1 /= SUMWN) .OR. ANY(T2 /= WLONN) .OR. ANY(T3 /= WLATN) .OR. ANY(T4 /= WCORN) .OR. ANY(T5 /= WKPMN) .OR. ANY(T6 /= WMPMN)) THEN
        ERROR STOP 'CTUWDRV LEFT OTHER WEIGHTS THAN THE CTUW CALLS'
      ENDIF
    ENDDO
    ! the flags of the general branch (ctuwupdt.F90:263-337)
    IF (CUR) THEN
      DO M = 1, NFRE_RED
        DO K = 1, NANG
          DO IC = 1, 2
            LLWLONN(K,M,IC) = ANY(WLONN(:,K,M,IC) > 0.0_JWRB)
            DO ICL = 1, 2
              LLWLATN(K,M,IC,ICL) = ANY(WLATN(:,K,M,IC,ICL) > 0.0_JWRB)
            ENDDO
          ENDDO
          DO ICR = 1, 4
            DO ICL = 1, 2
              LLWCORN(K,M,ICR,ICL) = ANY(WCORN(:,K,M,ICR,ICL) > 0.0_JWRB)
            ENDDO
          ENDDO
          DO IC = -1, 1
            LLWKPMN(K,M,IC) = ANY(WKPMN(:,K,M,IC) > 0.0_JWRB)
            LLWMPMN(K,M,IC) = ANY(WMPMN(:,K,M,IC) > 0.0_JWRB)
          ENDDO
        ENDDO
      ENDDO
    ENDIF
    ! the advection (propag_wam.F90:239-313)
    CALL PROPAGS2(F1, F3, 1_JWIM, N, 1_JWIM, N, NANG, 1_JWIM, NFRE_RED, 1_JWIM, NFRE_RED)
    IF (IFRELFMAX > 0 .AND. IFRELFMAX < NFRE_RED) THEN
      IF (NINT(REAL(IDELPRO, JWRB) / DELPRO_LF) /= 2) ERROR STOP 'NSTEP_LF'
      F1(1:N,:,1:IFRELFMAX) = F3(1:N,:,1:IFRELFMAX)
      CALL PROPAGS2(F1(:,:,1:IFRELFMAX+1), F3(:,:,1:IFRELFMAX), 1_JWIM, N, 1_JWIM, N, NANG, 1_JWIM, IFRELFMAX + 1, 1_JWIM, IFRELFMAX)
    ENDIF
    WRITE(12) REAL(F3(1:N,:,:), R8), REAL(THDD, R8), REAL(THDC, R8), REAL(SDOT, R8), FAIL1, CURMASK, FAIL, REAL(WLAT, R8), REAL(WCOR, R8)
    WRITE(12) REAL(SUMWN, R8), REAL(WLONN, R8), REAL(WLATN, R8), REAL(WCORN, R8), REAL(WKPMN, R8), REAL(WMPMN, R8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
CONTAINS
  SUBROUTINE SELECTORS      ! ctuwupdt.F90:93-161
    ALLOCATE(MPM(NFRE_RED,-1:1), KPM(NANG,-1:1), JXO(NANG,2), JYO(NANG,2), KCR(NANG,4))
    DO M = 1, NFRE_RED
      MPM(M,-1) = MAX(1,M-1); MPM(M,0) = M; MPM(M,1) = MIN(NFRE_RED,M+1)
    ENDDO
    DO K = 1, NANG
      KPM(K,-1) = MERGE(NANG, K-1, K-1 < 1); KPM(K,0) = K; KPM(K,1) = MERGE(1, K+1, K+1 > NANG)
      IF (COSTH(K) >= 0.0_JWRB) THEN
        JYO(K,:) = [1, 2]
        IF (SINTH(K) >= 0.0_JWRB) THEN
          JXO(K,:) = [1, 2]; KCR(K,:) = [3, 2, 4, 1]
        ELSE
          JXO(K,:) = [2, 1]; KCR(K,:) = [2, 3, 1, 4]
        ENDIF
      ELSE
        JYO(K,:) = [2, 1]
        IF (SINTH(K) >= 0.0_JWRB) THEN
          JXO(K,:) = [1, 2]; KCR(K,:) = [4, 1, 3, 2]
        ELSE
          JXO(K,:) = [2, 1]; KCR(K,:) = [1, 4, 2, 3]
        ENDIF
      ENDIF
    ENDDO
  END SUBROUTINE SELECTORS
END PROGRAM CTU_DRIVER
