! Driver of tools/make_golden_forcing.py: calls the reference's WAMWND, MICEP, CDUSTARZ0, WAMADSWSTAR, WAMCUR and OUTBETA on the records of a
! stream file and writes what they return.  It is built by oracle/ref_build.py::build_driver: the routines and the modules they use are the
! reference's own files, compiled unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90 for what other packages supply.
! The program fills the modules' variables from the file, so that the reference sees the constants of ecwam_amd/tables.py and
! tests/forcing_ref.py, the ones the device holds; what the reference declares a PARAMETER is compared with the file's value instead.  One
! module is the driver's own: YOWWIND, because the reference's RWFAC is a PARAMETER (0.5) and the recorded cases weigh the current with 1 and
! 0.625.  Two pieces of the seam are statements inside larger routines, not routines: the NEMO currents of getcurr.F90:168-181 and the WVBLOCK
! fill of wavemdl.F90:757-802.  The program restates those few lines around the reference's OUTBETA, as the start driver restates GETSPEC's
! fill loop.
! Input  (stream, little endian): NPTS, NX, NY (int32); IFROMIJ(NPTS), JFROMIJ(NPTS) (int32, 1-based); then records, each led by an int32 OP
!        (0 = the end), 24 real64 S and 16 int32 L:
!          S = G, GM1, ZPI, EPSUS, ZMISS, XKAPPA, XNLEV, RNUM, PRCHAR, ALPHAMIN, ALPHAMAX, ALPHA, WSPMIN, RWFAC, HICMIN, CITHRSH, SWAMPCITH, CDMAX,
!              C1CD, C2CD, P1CD, P2CD, CURRENT_MAX, (spare)
!          L = ICODE_WND, LLWSWAVE, LLWDWAVE, LWCOU, LWCUR, LRELWIND, IREFRA, IPARAMCI, LWNEMOCOUCIC, LWNEMOCOUCIT, LNEMOICEREST, LICETH, LICERUN,
!              LMASKICE, CLDOMAIN == 's', LLGCBZ0
!        and the arrays of the operation (real64):
!          1 GETWND:      FIELDG(NX,NY,13), UCUR, VCUR (NPTS), NEMO(NPTS,4), U10, US (NPTS; what the INOUT arguments hold before)
!                         -> ADS, THW, CICVR, U10, WSTAR, USTRA, VSTRA, US, CITH
!          2 CDUSTARZ0:   U10(NPTS) -> USTAR, Z0
!          3 WAMADSWSTAR: FIELDG -> AIRD, WSTAR, USTRA, VSTRA
!          4 WAMCUR:      FIELDG -> U, V
!          5 the NEMO currents: FIELDG, NEMO(NPTS,4) -> U, V
!          6 the WVBLOCK fill: FLAGS(4) = LWCOU2W, LWCOUHMF, LWSTOKES, LWFLUX and NWVFIELDS (int32); U10, USTAR, Z0M, Z0B, CHRNCK (NPTS);
!                         USTOKES, VSTOKES, PHIOCD, TAUOCXD, TAUOCYD, TAUICX, TAUICY, WSEMEAN, WSFMEAN (NPTS) -> WVBLOCK(NPTS,NWVFIELDS)
!        Every real is representable in the working precision.
! Output (stream): per record the columns listed, NPTS real64 each: the working-precision results, widened.
MODULE YOWWIND
  USE PARKIND_WAVE, ONLY : JWRB
  IMPLICIT NONE
  REAL(KIND=JWRB) :: WSPMIN, RWFAC
  LOGICAL :: LLWSWAVE, LLWDWAVE
END MODULE YOWWIND

PROGRAM FORCING_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB, JWRO
  USE YOWDRVTYPE, ONLY : FORCING_FIELDS, WVGRIDLOC
  USE YOWCOUP, ONLY : LWCOU, LWNEMOCOUCIC, LWNEMOCOUCIT, LLGCBZ0
  USE YOWPCONS, ONLY : G, GM1, ZPI, ZMISS, EPSUS, C1CD, C2CD, P1CD, P2CD, CDMAX
  USE YOWPHYS, ONLY : XKAPPA, XNLEV, RNUM, PRCHAR, ALPHAMIN, ALPHAMAX, ALPHA
  USE YOWSTAT, ONLY : IREFRA, LRELWIND
  USE YOWWIND, ONLY : WSPMIN, RWFAC, LLWSWAVE, LLWDWAVE
  USE YOWICE, ONLY : CITHRSH, HICMIN, LICERUN, LMASKICE, LICETH, LCIWA1
  USE YOWMAP, ONLY : NGX, NGY, CLDOMAIN
  USE YOWPARAM, ONLY : SWAMPCITH
  USE YOWNEMOFLDS, ONLY : LNEMOICEREST
  USE YOWCURR, ONLY : CURRENT_MAX
  USE YOWGRID, ONLY : NPROMA_WAM, NCHNK
  USE YOWMPP, ONLY : IRANK, NPROC
  IMPLICIT NONE
#include "outbeta.intfb.h"
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER(KIND=JWIM) :: NPTS, NX, NY, OP, L(16), FL(5), ICODE_WND, IPARAMCI, NWV, IJ, IX, JY, IFLD, J
  LOGICAL :: LWCUR, LWCOU2W, LWCOUHMF, LWSTOKES, LWFLUX
  REAL(KIND=R8) :: S(24)
  INTEGER(KIND=JWIM), ALLOCATABLE, TARGET :: IFROMIJ(:,:), JFROMIJ(:,:)
  REAL(KIND=R8), ALLOCATABLE :: G8(:,:,:), P8(:,:), N8(:,:), W8(:,:)
  REAL(KIND=JWRB), ALLOCATABLE, TARGET :: GF(:,:,:), FN(:,:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: P(:,:), O(:,:), CD(:), W(:,:)
  REAL(KIND=JWRO), ALLOCATABLE :: NEMO(:,:)
  TYPE(FORCING_FIELDS) :: FIELDG, FF_NOW
  TYPE(WVGRIDLOC) :: BLK2LOC
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) NPTS, NX, NY
  ALLOCATE(IFROMIJ(NPTS,1), JFROMIJ(NPTS,1), G8(NX,NY,13), GF(NX,NY,13), FN(NPTS,1,4), P8(NPTS,14), P(NPTS,14), N8(NPTS,4), NEMO(NPTS,4), O(NPTS,9), CD(NPTS))
  READ(11) IFROMIJ, JFROMIJ
  BLK2LOC%IFROMIJ => IFROMIJ
  BLK2LOC%JFROMIJ => JFROMIJ
  NGX = NX
  NGY = NY
  NPROMA_WAM = NPTS
  NCHNK = 1
  IRANK = 1
  NPROC = 1
  LCIWA1 = .FALSE.
  FIELDG%UWND => GF(:,:,1)
  FIELDG%VWND => GF(:,:,2)
  FIELDG%AIRD => GF(:,:,3)
  FIELDG%WSTAR => GF(:,:,4)
  FIELDG%CICOVER => GF(:,:,5)
  FIELDG%CITHICK => GF(:,:,6)
  FIELDG%USTRA => GF(:,:,7)
  FIELDG%VSTRA => GF(:,:,8)
  FIELDG%WSWAVE => GF(:,:,9)
  FIELDG%WDWAVE => GF(:,:,10)
  FIELDG%LKFR => GF(:,:,11)
  FIELDG%UCUR => GF(:,:,12)
  FIELDG%VCUR => GF(:,:,13)
  FF_NOW%AIRD => FN(:,:,1)
  FF_NOW%WSTAR => FN(:,:,2)
  FF_NOW%USTRA => FN(:,:,3)
  FF_NOW%VSTRA => FN(:,:,4)
  DO
    READ(11) OP
    IF (OP == 0) EXIT
    READ(11) S, L
    G = REAL(S(1), JWRB)
    GM1 = REAL(S(2), JWRB)
    ZPI = REAL(S(3), JWRB)
    IF (REAL(S(4), JWRB) /= EPSUS) ERROR STOP 'EPSUS'
    ZMISS = REAL(S(5), JWRB)
    IF (REAL(S(6), JWRB) /= XKAPPA) ERROR STOP 'XKAPPA'
    IF (REAL(S(7), JWRB) /= XNLEV) ERROR STOP 'XNLEV'
    RNUM = REAL(S(8), JWRB)
    PRCHAR = REAL(S(9), JWRB)
    ALPHAMIN = REAL(S(10), JWRB)
    IF (REAL(S(11), JWRB) /= ALPHAMAX) ERROR STOP 'ALPHAMAX'
    ALPHA = REAL(S(12), JWRB)
    WSPMIN = REAL(S(13), JWRB)
    RWFAC = REAL(S(14), JWRB)
    IF (REAL(S(15), JWRB) /= HICMIN) ERROR STOP 'HICMIN'
    CITHRSH = REAL(S(16), JWRB)
    SWAMPCITH = REAL(S(17), JWRB)
    IF (REAL(S(18), JWRB) /= CDMAX) ERROR STOP 'CDMAX'
    IF (REAL(S(19), JWRB) /= C1CD) ERROR STOP 'C1CD'
    IF (REAL(S(20), JWRB) /= C2CD) ERROR STOP 'C2CD'
    IF (REAL(S(21), JWRB) /= P1CD) ERROR STOP 'P1CD'
    IF (REAL(S(22), JWRB) /= P2CD) ERROR STOP 'P2CD'
    IF (REAL(S(23), JWRB) /= CURRENT_MAX) ERROR STOP 'CURRENT_MAX'
    ICODE_WND = L(1)
    LLWSWAVE = L(2) /= 0
    LLWDWAVE = L(3) /= 0
    LWCOU = L(4) /= 0
    LWCUR = L(5) /= 0
    LRELWIND = L(6) /= 0
    IREFRA = L(7)
    IPARAMCI = L(8)
    LWNEMOCOUCIC = L(9) /= 0
    LWNEMOCOUCIT = L(10) /= 0
    LNEMOICEREST = L(11) /= 0
    LICETH = L(12) /= 0
    LICERUN = L(13) /= 0
    LMASKICE = L(14) /= 0
    CLDOMAIN = MERGE('s', 'g', L(15) /= 0)
    LLGCBZ0 = L(16) /= 0
    IF (OP == 1) THEN
      READ(11) G8, P8(:,1:2), N8, P8(:,3:4)
      GF = REAL(G8, JWRB)
      P(:,1:4) = REAL(P8(:,1:4), JWRB)
      NEMO = REAL(N8, JWRO)
      O = 0.0_JWRB
      O(:,4) = P(:,3)
      O(:,8) = P(:,4)
      CALL WAMWND(1_JWIM, NPTS, IFROMIJ(:,1), JFROMIJ(:,1), 1_JWIM, NX, 1_JWIM, NY, FIELDG, P(:,1), P(:,2), O(:,4), O(:,8), O(:,2), O(:,1), O(:,5),  &
 &                O(:,9), O(:,6), O(:,7), LWCUR, ICODE_WND)
      CALL MICEP(IPARAMCI, 1_JWIM, NPTS, IFROMIJ(:,1), JFROMIJ(:,1), 1_JWIM, NX, 1_JWIM, NY, FIELDG, O(:,3), O(:,9), NEMO(:,1), NEMO(:,2))
      WRITE(12) REAL(O, R8)
    ELSEIF (OP == 2) THEN
      READ(11) P8(:,1)
      P(:,1) = REAL(P8(:,1), JWRB)
      CALL CDUSTARZ0(1_JWIM, NPTS, P(:,1), XNLEV, CD, O(:,1), O(:,2))
      WRITE(12) REAL(O(:,1:2), R8)
    ELSEIF (OP == 3) THEN
      READ(11) G8
      GF = REAL(G8, JWRB)
      FN = 0.0_JWRB
      CALL WAMADSWSTAR(1_JWIM, NX, 1_JWIM, NY, FIELDG, BLK2LOC, FF_NOW)
      WRITE(12) REAL(FN(:,1,:), R8)
    ELSEIF (OP == 4) THEN
      READ(11) G8
      GF = REAL(G8, JWRB)
      CALL WAMCUR(1_JWIM, NX, 1_JWIM, NY, FIELDG, 1_JWIM, NPTS, IFROMIJ(:,1), JFROMIJ(:,1), O(:,1), O(:,2))
      WRITE(12) REAL(O(:,1:2), R8)
    ELSEIF (OP == 5) THEN
      READ(11) G8, N8
      GF = REAL(G8, JWRB)
      NEMO = REAL(N8, JWRO)
      DO IJ = 1, NPTS      ! the currents of NEMO where the point is open ocean, clipped in NEMO's kind; none over lakes and land
        IX = IFROMIJ(IJ,1)
        JY = JFROMIJ(IJ,1)
        IF (FIELDG%LKFR(IX,JY) <= 0.0_JWRB) THEN
          O(IJ,1) = SIGN(MIN(ABS(NEMO(IJ,3)), REAL(CURRENT_MAX, JWRO)), NEMO(IJ,3))
          O(IJ,2) = SIGN(MIN(ABS(NEMO(IJ,4)), REAL(CURRENT_MAX, JWRO)), NEMO(IJ,4))
        ELSE
          O(IJ,1) = 0.0_JWRB
          O(IJ,2) = 0.0_JWRB
        ENDIF
      ENDDO
      WRITE(12) REAL(O(:,1:2), R8)
    ELSE
      READ(11) FL
      LWCOU2W = FL(1) /= 0
      LWCOUHMF = FL(2) /= 0
      LWSTOKES = FL(3) /= 0
      LWFLUX = FL(4) /= 0
      NWV = FL(5)
      READ(11) P8
      P = REAL(P8, JWRB)
      ALLOCATE(W(NPTS,NWV), W8(NPTS,NWV))
      IF (LWCOU2W) THEN
        CALL OUTBETA(1_JWIM, NPTS, P(:,1), P(:,2), P(:,3), P(:,4), P(:,5), O(:,1), O(:,2))
      ELSE
        O(:,1) = PRCHAR
      ENDIF
      IFLD = 1      ! the fields in the order of the coupling interface
      W(:,IFLD) = O(:,1)
      IF (LWCOUHMF) THEN
        IFLD = IFLD + 1
        W(:,IFLD) = O(:,2)
      ENDIF
      IF (LWSTOKES) THEN
        DO J = 6, 7
          IFLD = IFLD + 1
          W(:,IFLD) = P(:,J)
        ENDDO
      ENDIF
      IF (LWFLUX) THEN
        DO J = 8, 14
          IFLD = IFLD + 1
          W(:,IFLD) = P(:,J)
        ENDDO
      ENDIF
      DO J = IFLD + 1, NWV
        W(:,J) = 0.0_JWRB
      ENDDO
      W8 = REAL(W, R8)
      WRITE(12) W8
      DEALLOCATE(W, W8)
    ENDIF
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM FORCING_DRIVER
